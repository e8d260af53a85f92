"""The streaming kernels of pgl_elementwise.hip and the shared walk over Psi of pgl_obs.h entry point by entry point, through the C ABI alone
(pyglm_amd._lib.call; no engine): pgl_design_matrix, pgl_transpose, pgl_pg_loglik, pgl_pg_loglik_ex, pgl_gaussian_stats, pgl_summary_colsum,
pgl_assemble_posterior, pgl_scaled_gram.  tests/_streaming_cases.py holds the cases, the CPU references and the restated launch geometry the
shapes are chosen from; tests/test_streaming_cases_host.py checks those without a GPU.

Every buffer a kernel writes carries guards -- padding columns up to the leading dimension, rows past T or D, one whole slot or row after the
last -- of NaN, compared as bit patterns afterwards; whatever must not be read (padding columns of S, Y, Psi, bias, param, hooks, the border
columns beyond D, inv_eta past nz) is NaN and the outputs must be finite."""
import numpy as np
import pytest

from tests import _streaming_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)      # (a copy: views of read-only arrays come here too)


def _host(t):
    return t.cpu().numpy()


def _call(name, **kw):
    import torch
    from pyglm_amd._lib import call
    call(name, hip_stream=None, **kw)
    torch.cuda.synchronize()


def _status(name, **kw):
    """(return value, pgl_last_error()) of an entry that is expected to refuse its arguments"""
    import torch
    from pyglm_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, name)(*[dict(kw, hip_stream=None)[k] for k in _lib.PARAMS[name]])
    torch.cuda.synchronize()
    return rc, lib.pgl_last_error().decode()


def _ptr(t):
    from pyglm_amd._lib import ptr
    return ptr(t)


# ================================================================================================================ A. pgl_design_matrix
def _design(c, S_d, basis_d, X_d, Xt_d, T, clip):
    _call("pgl_design_matrix", S=_ptr(S_d), lds=c["lds"], basis=_ptr(basis_d), X=_ptr(X_d), ldx=c["ldx"], Xt=_ptr(Xt_d), ldxt=c["ldxt"] if Xt_d is not None else 0,
          T=T, N=c["N"], B=c["B"], R=c["R"], clip=clip)


def _check_design(kind, T, N, B, R, clips=(0, 1)):
    c = S.design_case(kind, T, N, B, R)
    D, what = c["D"], "%s design (T, N, B, R) = %s" % (kind, (T, N, B, R))
    S_d, basis_d = _dev(c["S_buf"]), _dev(c["basis"])
    for clip in clips:
        ref, mag = S.design_ref(c["S"], c["basis"], clip)
        for with_xt in (False, True):
            X0, Xt0 = np.full((c["x_rows"], c["ldx"]), np.nan), np.full((c["xt_rows"], c["ldxt"]), np.nan)
            X_d, Xt_d = _dev(X0), _dev(Xt0) if with_xt else None
            _design(c, S_d, basis_d, X_d, Xt_d, T, clip)
            X = _host(X_d)
            got = X[:T, :D + 1]
            if kind == "exact":
                S.same_bits(got, ref.astype(np.float64), what)
            else:
                assert np.isfinite(got).all(), what
                err = np.abs(got.astype(S.LD) - ref)
                assert (err <= S.design_bound(mag, R)).all(), "%s: worst |err| / bound = %.3g" % (what, float((err / np.where(mag > 0, S.design_bound(mag, R), 1)).max()))
            S.same_bits(got[0, :D], np.zeros(D), what + ": row 0")
            S.same_bits(got[:, D], np.ones(T), what + ": the ones column")
            if clip:
                assert not (got < 0).any() and not np.signbit(got).any()
            expect = X0.copy()
            expect[:T, :D + 1] = got
            S.same_bits(X, expect, what + ": X outside [T][D + 1]")
            if with_xt:
                Xt = _host(Xt_d)
                expect = Xt0.copy()
                expect[:D + 1, :T] = got.T
                S.same_bits(Xt, expect, what + ": Xt against X transposed, and outside [D + 1][T]")
        if clip == 0:
            # a block of rows [r0, r1) with h = min(R, r0) rows of history, as simulate.py forms X: the rows of the whole, bit for bit
            for r0, r1 in S.history_blocks(T, R):
                h = min(R, r0)
                Tb = r1 - r0 + h
                Xs0 = np.full((Tb + 1, c["ldx"]), np.nan)
                Xs_d = _dev(Xs0)
                _design(c, S_d[r0 - h:], basis_d, Xs_d, None, Tb, 0)
                Xs = _host(Xs_d)
                S.same_bits(Xs[h:Tb, :D], got[r0:r1, :D], what + ": rows [%d, %d) with %d rows of history" % (r0, r1, h))
                assert np.isnan(Xs[Tb]).all() and np.isnan(Xs[:, D + 1:]).all()


@pytest.mark.parametrize("T,N,B,R", S.DESIGN_SHAPES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_design_matrix(kind, T, N, B, R):
    """both clips, Xt NULL and given, lds > N, ldx > N B + 1, ldxt > T, X and Xt with rows past T and D + 1: bit-equal to NumPy on dyadic
    operands, within (R + 2) 2^-53 sum |basis| |S| on real ones; row 0 zero, the ones column 1, Xt = X' bit for bit, and a block of rows
    computed with its history equal to the rows of the whole"""
    _check_design(kind, T, N, B, R)


def test_design_matrix_basis_past_64_kib_of_lds():
    """R * B * 8 = 65 792 bytes: the launcher raises the kernel's dynamic-LDS limit (pgl_grow_dynamic_lds) for a basis beyond 64 KiB"""
    T, N, B, R = S.DESIGN_LDS_SHAPE
    assert S.LDS_DEFAULT < S.conv_lds_bytes(R, B) <= S.LDS_MAX
    _check_design("exact", T, N, B, R, clips=(0,))


def _refused(T, N, B, R):
    c = S.design_case("exact", T, N, min(B, 32), R)
    c.update(B=B, D=N * B, ldx=N * B + 4)
    X0, Xt0 = np.full((T + 2, c["ldx"]), np.nan), np.full((N * B + 3, c["ldxt"]), np.nan)
    S_d, basis_d, X_d, Xt_d = _dev(c["S_buf"]), _dev(np.ones((R, B))), _dev(X0), _dev(Xt0)
    rc, msg = _status("pgl_design_matrix", S=_ptr(S_d), lds=c["lds"], basis=_ptr(basis_d), X=_ptr(X_d), ldx=c["ldx"], Xt=_ptr(Xt_d), ldxt=c["ldxt"], T=T, N=N,
                      B=B, R=R, clip=0)
    S.same_bits(_host(X_d), X0, "a refused call wrote X")
    S.same_bits(_host(Xt_d), Xt0, "a refused call wrote Xt")
    return rc, msg


def test_design_matrix_refuses_b_33():
    rc, msg = _refused(5, 3, 33, 4)
    assert rc == S.PGL_ERR_ARG and "33" in msg


def test_design_matrix_refuses_a_basis_beyond_160_kib_of_lds():
    T, N, B, R = S.DESIGN_LDS_REFUSED
    assert S.conv_lds_bytes(R, B) > S.LDS_MAX
    rc, msg = _refused(T, N, B, R)
    assert rc == S.PGL_ERR_ARG and "R=%d" % R in msg and "B=%d" % B in msg


# ================================================================================================================ B. pgl_transpose
@pytest.mark.parametrize("rows", sorted({r for r, _ in S.TRANSPOSE_SHAPES}))
def test_transpose(rows):
    """32 x 32 tiles, ragged on either side: the NumPy transpose bit for bit, nothing outside dst[:cols, :rows] touched, no NaN from outside
    src[:rows, :cols] in the output"""
    for cols in sorted({c for r, c in S.TRANSPOSE_SHAPES if r == rows}):
        c = S.transpose_case(rows, cols)
        src, dst = _dev(c["src"]), _dev(c["dst"])
        _call("pgl_transpose", src=_ptr(src), ld_src=c["ld_src"], dst=_ptr(dst), ld_dst=c["ld_dst"], rows=rows, cols=cols)
        expect = c["dst"].copy()
        expect[:cols, :rows] = c["values"].T
        S.same_bits(_host(dst), expect, "transpose %d x %d" % (rows, cols))
        S.same_bits(_host(src), c["src"], "transpose %d x %d: the source" % (rows, cols))


# ================================================================================================================ C. the pass over Psi
def _draws(b, psi_out, neuron0, elem0):
    """what pgl_pg_draw returns for (b, psi_out) [T][nloc], column n on the stream of neuron neuron0 + n in sweep SWEEP, element elem0 + t"""
    import torch
    from pyglm_amd._lib import call
    T, nloc = psi_out.shape
    bT, zT = _dev(np.broadcast_to(b, (T, nloc)).T), _dev(psi_out.T)
    out = torch.full((nloc, T), float("nan"), dtype=torch.float64, device=DEV)
    for n in range(nloc):
        call("pgl_pg_draw", b=_ptr(bT[n]), z=_ptr(zT[n]), out=_ptr(out[n]), len=T, seed=S.SEED, stream=S.pg_stream(S.SWEEP, neuron0 + n), elem0=elem0,
             hip_stream=None)
    torch.cuda.synchronize()
    return _host(out).T.copy()


class _Pass:
    """the device buffers of one case, fresh: Psi, Y, bias, param, hooks, inv_eta as the case poisons them, Omega / Kappa, llpart and ll_out NaN"""

    def __init__(self, c, ll0=None, with_ok=True):
        T, nloc = c["T"], c["nloc"]
        self.c, self.nblk = c, S.psi_row_blocks(T)
        self.Psi, self.Y, self.bias = _dev(c["Psi_buf"]), _dev(c["Y_buf"]), _dev(c["bias_buf"])
        self.param = None if c.get("param_buf") is None else _dev(c["param_buf"])
        self.hooks = None if c.get("hooks") is None else _dev(c["hooks"])
        self.inv_eta = None if c.get("inv_eta_buf") is None else _dev(c["inv_eta_buf"])
        self.llpart0 = np.full((self.nblk + 1, nloc), np.nan)                # exactly pgl_pg_loglik_partials(T) * nloc doubles, and a guard row
        self.ll0 = np.full(nloc + 2, np.nan)
        if ll0 is not None:
            self.ll0[:nloc] = ll0
        self.llpart, self.ll = _dev(self.llpart0), _dev(self.ll0)
        self.Omega = self.Kappa = self.OK = None
        if with_ok and c["layout"] == "production":
            self.OK0 = np.full((c["ok_rows"], 2 * c["ldn"]), np.nan)
            self.OK = _dev(self.OK0)
            self.Omega, self.Kappa = self.OK.view(-1), self.OK.view(-1)[c["ldn"]:]
        elif with_ok:
            self.O0, self.K0 = np.full((c["ok_rows"], c["ldo"]), np.nan), np.full((c["ok_rows"], c["ldk"]), np.nan)
            self.Omega, self.Kappa = _dev(self.O0), _dev(self.K0)

    def run(self, entry="pgl_pg_loglik_ex", accumulate=0, bias=True, col=(0, None), rows=(0, None), neuron0=S.NEURON0, elem0=S.ELEM0, hooks=None, obs=None):
        """the entry on columns [col) and rows [rows) of the buffers (the whole by default), neuron0 and elem0 as given"""
        from pyglm_amd import _lib
        c = self.c
        c0, c1 = col[0], c["nloc"] if col[1] is None else col[1]
        r0, r1 = rows[0], c["T"] if rows[1] is None else rows[1]
        at = lambda t, ld: None if t is None else _ptr(t.view(-1)[r0 * ld + c0:])
        assert _lib.load().pgl_pg_loglik_partials(r1 - r0) == S.psi_row_blocks(r1 - r0)
        kw = dict(Psi=at(self.Psi, c["ldpsi"]), ldpsi=c["ldpsi"], bias=at(self.bias, 0) if bias else None, Y=at(self.Y, c["ldy"]), ldy=c["ldy"],
                  Omega=at(self.Omega, c["ldo"]), ldo=c["ldo"], Kappa=at(self.Kappa, c["ldk"]), ldk=c["ldk"], accumulate=accumulate, T=r1 - r0, nloc=c1 - c0)
        part = _ptr(self.llpart.view(-1)[self.nblk * c0:])                   # (a shard's partials: its own [blocks][c1 - c0] inside the buffer)
        if entry == "pgl_gaussian_stats":
            _call(entry, inv_eta=at(self.inv_eta, 0), part=part, sse_out=at(self.ll, 0), **kw)
            return self
        kw.update(llpart=part, ll_out=at(self.ll, 0), obs=c["obs"] if obs is None else obs, xi=c["xi"], seed=S.SEED, sweep=S.SWEEP, neuron0=neuron0 + c0,
                  elem0=elem0 + r0)
        if entry == "pgl_pg_loglik_ex":
            hk = self.hooks if hooks is None else hooks
            kw.update(param=at(self.param, 0), hooks=None if hk is None else _ptr(hk.view(-1)[r0 * 3 * c["ldh"] + c0:]), ldh=c["ldh"])
        _call(entry, **kw)
        return self

    def out(self):
        """host copies: Psi, Omega, Kappa [T][nloc] and the whole buffers, llpart, ll"""
        c = self.c
        T, nloc = c["T"], c["nloc"]
        o = dict(Psi_buf=_host(self.Psi), llpart_buf=_host(self.llpart), ll_buf=_host(self.ll))
        o.update(Psi=o["Psi_buf"][:T, :nloc], llpart=o["llpart_buf"][:self.nblk], ll=o["ll_buf"][:nloc])
        if self.OK is not None:
            o["OK_buf"] = _host(self.OK)
            o.update(Omega=o["OK_buf"][:T, :nloc], Kappa=o["OK_buf"][:T, c["ldn"]:c["ldn"] + nloc])
        elif self.Omega is not None:
            o.update(Omega_buf=_host(self.Omega), Kappa_buf=_host(self.Kappa))
            o.update(Omega=o["Omega_buf"][:T, :nloc], Kappa=o["Kappa_buf"][:T, :nloc])
        return o

    def check_guards(self, o, what):
        """everything outside [T][nloc] of Psi, Omega, Kappa, the guard row of llpart and the tail of ll_out: the bits they had on entry"""
        c = self.c
        T, nloc = c["T"], c["nloc"]

        def outside(buf, before, blocks, name):
            expect = before.copy()
            for rs, cs in blocks:
                expect[rs, cs] = buf[rs, cs]
            S.same_bits(buf, expect, "%s: %s outside what the pass writes" % (what, name))
        cell = (slice(0, T), slice(0, nloc))
        outside(o["Psi_buf"], c["Psi_buf"], [cell], "Psi")
        outside(o["llpart_buf"], self.llpart0, [(slice(0, self.nblk), slice(None))], "llpart")
        S.same_bits(o["ll_buf"][nloc:], self.ll0[nloc:], what + ": ll_out past nloc")
        if self.OK is not None:
            outside(o["OK_buf"], self.OK0, [cell, (slice(0, T), slice(c["ldn"], c["ldn"] + nloc))], "[Omega | Kappa] (rows >= T, padding columns)")
        elif self.Omega is not None:
            outside(o["Omega_buf"], self.O0, [cell], "Omega")
            outside(o["Kappa_buf"], self.K0, [cell], "Kappa")
        for k in ("Psi", "Omega", "Kappa", "llpart", "ll"):
            assert k not in o or np.isfinite(o[k]).all(), "%s: %s is not finite (a poisoned cell was read)" % (what, k)


def _fold_terms(c, psi_out):
    """pgl_summary_fold with k = 1 on zeroed accumulators over psi_out (bias already added): (l_mean [T][nloc] = the cell's term l exactly, its ll_out)"""
    T, nloc, ldn = c["T"], c["nloc"], c["ldpsi"]
    Psi, Y = _dev(S.guarded(psi_out, T + 1, ldn)), _dev(S.guarded(c["Y"], T + 1, ldn))
    acc0 = S.guarded(np.zeros((T, nloc)), T + 1, ldn)
    acc = [_dev(acc0) for _ in range(4)]
    p = _Pass(c, with_ok=False)
    _call("pgl_summary_fold", Psi=_ptr(Psi), ldn=ldn, bias=None, Y=_ptr(Y), llpart=_ptr(p.llpart), ll_out=_ptr(p.ll), accumulate=0, T=T, nloc=nloc, obs=c["obs"],
          xi=c.get("xi", 0.0), param=_ptr(p.param), hooks=_ptr(p.hooks), ldh=c.get("ldh", ldn), inv_eta=_ptr(p.inv_eta), rate_mean=None, rate_M2=None, link=None,
          link0=0, link_par=None, link_par0=0.0, l_mean=_ptr(acc[0]), l_M2=_ptr(acc[1]), lse_m=_ptr(acc[2]), lse_s=_ptr(acc[3]), k=1)
    lmean = _host(acc[0])
    expect = acc0.copy()
    expect[:T, :nloc] = lmean[:T, :nloc]
    S.same_bits(lmean, expect, "l_mean outside [T][nloc]")
    S.same_bits(_host(Psi), S.guarded(psi_out, T + 1, ldn), "the fold wrote Psi")
    return lmean[:T, :nloc].copy(), _host(p.ll)[:nloc], _host(p.llpart)[:p.nblk]


def _colsum(V, accumulate=0, out0=None):
    T, nloc = V.shape
    nblk = S.psi_row_blocks(T)
    Vd, part = _dev(S.guarded(V, T + 1, nloc + 6)), _dev(np.full((nblk + 1, nloc), np.nan))
    out = _dev(S.guarded_vec(np.zeros(nloc) if out0 is None else out0, nloc + 2))
    _call("pgl_summary_colsum", V=_ptr(Vd), ldv=nloc + 6, T=T, nloc=nloc, part=_ptr(part), out=_ptr(out), accumulate=accumulate)
    part, out = _host(part), _host(out)
    assert np.isnan(part[nblk]).all() and np.isnan(out[nloc:]).all()
    return out[:nloc], part[:nblk]


def _check_order(terms, c, first, fold_ll, fold_part, rerun, what):
    """the order of addition, from the device's own terms: ll_out of the entry and of the fold, pgl_summary_colsum of the terms, llpart, and
    both values of `accumulate` with ll_out preloaded -- all the bits of the NumPy emulation"""
    nloc = c["nloc"]
    out, part = S.emulate_reduction(terms)
    S.same_bits(first["ll"], out, what + ": ll_out against the emulated order of addition")
    S.same_bits(first["llpart"], part, what + ": llpart against the emulated partials")
    S.same_bits(fold_ll, out, what + ": ll_out of pgl_summary_fold")
    S.same_bits(fold_part, part, what + ": llpart of pgl_summary_fold")
    cs, cpart = _colsum(terms)
    S.same_bits(cs, out, what + ": pgl_summary_colsum of the terms")
    S.same_bits(cpart, part, what + ": the partials of pgl_summary_colsum")
    ll0 = np.random.default_rng(9).standard_normal(nloc) * 100
    S.same_bits(_colsum(terms, 1, ll0)[0], ll0 + out, what + ": pgl_summary_colsum accumulating")
    for accumulate in (0, 1):
        o = rerun(accumulate, ll0)
        S.same_bits(o["ll"], ll0 + out if accumulate else out, what + ": accumulate = %d on a preloaded ll_out" % accumulate)
        for k in ("Psi", "Omega", "Kappa", "llpart"):
            S.same_bits(o[k], first[k], what + ": %s of a second call" % k)


RATIOS = {}      # variant -> the largest |l - reference| in units of 2^-53 (sum of magnitudes), against the cap of 16


@pytest.mark.parametrize("T,nloc", S.PSI_SHAPES)
@pytest.mark.parametrize("variant", list(S.PSI_VARIANTS))
def test_pg_pass(variant, T, nloc):
    """pgl_pg_loglik_ex cell by cell and sum by sum.  Largest per-cell error observed on an MI355X, in the units of which the cap allows 16
    (2^-53 times the sum of the magnitudes that enter the term), over all shapes of a variant:
        bernoulli 1.92   negbin 1.71   negbin_param 2.20   binomial 1.29   binomial_param 1.91   hooks 1.85
    (printed per case; run with -s)"""
    c = S.psi_case(T, nloc, variant)
    what = "%s T = %d nloc = %d (%s walk, %s layout)" % (variant, T, nloc, "narrow" if S.psi_narrow(nloc, c["obs"]) else "wide", c["layout"])
    p = _Pass(c).run()
    o = p.out()
    p.check_guards(o, what)
    psi_out = c["psi"] + c["bias"]
    S.same_bits(o["Psi"], psi_out, what + ": Psi + bias")
    S.same_bits(o["Kappa"], c["a"] - 0.5 * c["b"], what + ": Kappa = a - b / 2")
    S.same_bits(o["Omega"], _draws(c["b"], psi_out, S.NEURON0, S.ELEM0), what + ": Omega against pgl_pg_draw on (seed, sweep, neuron0 + n, elem0 + t)")
    # the per-cell term
    terms, fold_ll, fold_part = _fold_terms(c, psi_out)
    l, cap = S.ll_reference(c, psi_out)
    ratio = float((np.abs(terms.astype(S.LD) - l) / np.where(cap > 0, cap, 1)).max() * 16)
    RATIOS[variant] = max(RATIOS.get(variant, 0.0), ratio)
    print("%s: largest per-cell error %.3g units of the 16 allowed (the variant so far: %.3g)" % (what, ratio, RATIOS[variant]))
    assert np.isfinite(terms).all() and (np.abs(terms.astype(S.LD) - l) <= cap).all(), "%s: a cell's term is %.3g units off, 16 allowed" % (what, ratio)
    # the order of addition
    _check_order(terms, c, o, fold_ll, fold_part, lambda accumulate, ll0: _Pass(c, ll0=ll0).run(accumulate=accumulate).out(), what)
    # bias = NULL: Psi unchanged;  Omega = Kappa = NULL: only Psi, llpart and ll_out are written
    q = _Pass(dict(c, psi=psi_out, Psi_buf=S.guarded(psi_out, T + 1, c["ldpsi"])), with_ok=False).run(bias=False)
    oq = q.out()
    q.check_guards(oq, what + ", likelihood only")
    S.same_bits(oq["Psi"], psi_out, what + ": Psi with bias = NULL")
    S.same_bits(oq["ll"], o["ll"], what + ": ll_out of the likelihood-only pass")
    S.same_bits(oq["llpart"], o["llpart"], what + ": llpart of the likelihood-only pass")


@pytest.mark.parametrize("T,nloc", S.GAUSS_SHAPES)
def test_gaussian_pass(T, nloc):
    """pgl_gaussian_stats (always the wide walk): Psi + bias, Omega = 1 / eta, Kappa = y / eta per cell, and the sum of squared residuals in the
    order of the log-likelihood's reduction, with the (exactly representable) squares as terms"""
    c = S.gauss_case(T, nloc)
    what = "gaussian T = %d nloc = %d" % (T, nloc)
    assert not S.psi_narrow(nloc, 2)
    p = _Pass(c).run("pgl_gaussian_stats")
    o = p.out()
    p.check_guards(o, what)
    psi_out = c["psi"] + c["bias"]
    S.same_bits(o["Psi"], psi_out, what + ": Psi + bias")
    S.same_bits(o["Kappa"], c["Y"] * c["inv_eta"][None, :], what + ": Kappa = y / eta")
    S.same_bits(o["Omega"], np.broadcast_to(c["inv_eta"], (T, nloc)), what + ": Omega = 1 / eta")
    terms = c["r"] * c["r"]
    _, fold_ll, fold_part = _fold_terms(c, psi_out)
    _check_order(terms, c, o, fold_ll, fold_part, lambda accumulate, ll0: _Pass(c, ll0=ll0).run("pgl_gaussian_stats", accumulate=accumulate).out(), what)
    q = _Pass(dict(c, psi=psi_out, Psi_buf=S.guarded(psi_out, T + 1, c["ldpsi"])), with_ok=False).run("pgl_gaussian_stats", bias=False)
    oq = q.out()
    q.check_guards(oq, what + ", statistics only")
    S.same_bits(oq["Psi"], psi_out, what + ": Psi with bias = NULL")
    S.same_bits(oq["ll"], o["ll"], what + ": sse of the statistics-only pass")


@pytest.mark.parametrize("variant", ["bernoulli", "negbin_param", "hooks"])
def test_a_neuron_has_the_same_bits_whatever_the_shard(variant):
    """96 neurons in one wide call; as [0, 64) wide + [64, 96) narrow; as [0, 40) + [40, 96), both narrow -- each with neuron0 at its offset"""
    c = S.psi_case(130, 96, variant)
    whole = _Pass(c).run().out()
    for cuts in ((0, 64, 96), (0, 40, 96)):
        p = _Pass(c)
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            assert S.psi_narrow(c1 - c0, c["obs"]) == (c1 - c0 < 64)
            p.run(col=(c0, c1))
        o = p.out()
        for k in ("Psi", "Omega", "Kappa", "ll"):
            S.same_bits(o[k], whole[k], "%s, shards %s: %s" % (variant, cuts, k))
        for k in ("Psi_buf", "OK_buf", "Omega_buf", "Kappa_buf", "ll_buf"):
            if k in o:
                S.same_bits(o[k], whole[k], "%s, shards %s: %s" % (variant, cuts, k))


@pytest.mark.parametrize("nloc", [5, 65])
@pytest.mark.parametrize("variant", ["bernoulli", "negbin"])
def test_pg_loglik_is_the_extended_entry_without_param_and_hooks(variant, nloc):
    c = S.psi_case(130, nloc, variant)
    a, b = _Pass(c).run("pgl_pg_loglik").out(), _Pass(c).run("pgl_pg_loglik_ex").out()
    assert sorted(a) == sorted(b)
    for k in a:
        S.same_bits(a[k], b[k], "%s nloc = %d: %s" % (variant, nloc, k))


@pytest.mark.parametrize("nloc", [5, 65])
def test_hooks_of_the_bernoulli_model_are_the_bernoulli_model(nloc):
    c = S.psi_case(130, nloc, "bernoulli")
    a = _Pass(c).run().out()
    b = _Pass(c).run(hooks=_dev(S.hooks_of_bernoulli(c)), obs=4).out()
    for k in a:
        S.same_bits(a[k], b[k], "hooks (y, 1, 0) nloc = %d: %s" % (nloc, k))


@pytest.mark.parametrize("nloc", [5, 65])
@pytest.mark.parametrize("variant", ["negbin_param", "hooks"])
def test_rows_in_two_calls(variant, nloc):
    """rows [0, T1) with elem0 and rows [T1, T) with elem0 + T1 and accumulate = 1: the Omega (and Psi, Kappa) of one call bit for bit; ll within
    (T / 64 + 20) 2^-53 sum |l| (another order of addition)"""
    T, T1 = 257, 100
    c = S.psi_case(T, nloc, variant)
    whole = _Pass(c).run().out()
    p = _Pass(c).run(rows=(0, T1))
    first = p.out()
    S.same_bits(first["Psi_buf"][T1:], c["Psi_buf"][T1:], "rows past T1 of the first call")
    p.llpart.copy_(_dev(p.llpart0))
    o = p.run(rows=(T1, T), accumulate=1).out()
    for k in ("Psi_buf", "Omega_buf", "Kappa_buf"):
        S.same_bits(o[k], whole[k], "%s nloc = %d: %s of two calls" % (variant, nloc, k))
    l, _ = S.ll_reference(c, c["psi"] + c["bias"])
    bound = (T / 64 + 20) * S.U * np.abs(l).sum(axis=0).astype(np.float64)
    assert (np.abs(o["ll"] - whole["ll"]) <= bound).all(), "ll of two calls: worst %.3g of the bound" % float((np.abs(o["ll"] - whole["ll"]) / bound).max())


# ================================================================================================================ D. pgl_assemble_posterior
@pytest.mark.parametrize("N,B", S.ASSEMBLE_SHAPES)
@pytest.mark.parametrize("nb", S.ASSEMBLE_NB)
def test_assemble_posterior(nb, N, B):
    """J NaN but for the lower triangles of the diagonal blocks: those + Jw, the bias row D, the potential row D + 1, and every other cell -- the
    upper triangles, columns and rows past D + 1, the slot after nb -- the bits it had; the dense prior, and the label / table prior, which equals
    the dense prior it expands to bit for bit"""
    c = S.assemble_case(N, B, nb)
    D = c["D"]
    bo, bk, Jb, hb = _dev(c["bo"]), _dev(c["bk"]), _dev(c["Jb"]), _dev(c["hb"])

    def run(Jw, hw, label):
        J, Jw_d, hw_d, label_d = _dev(c["J"]), _dev(Jw), _dev(hw), None if label is None else _dev(label, np.int32)
        _call("pgl_assemble_posterior", J=_ptr(J), ldj=c["ldj"], strideJ=c["rows"] * c["ldj"], border_omega=_ptr(bo), border_kappa=_ptr(bk), ldb=c["ldb"],
              Jw=_ptr(Jw_d), hw=_ptr(hw_d), label=_ptr(label_d), Jb=_ptr(Jb), hb=_ptr(hb), nb=nb, N=N, B=B)
        return _host(J)
    what = "assembly N = %d B = %d nb = %d" % (N, B, nb)
    dense = run(c["Jw"], c["hw"], None)
    S.same_bits(dense, S.assemble_ref(c, c["Jw"], c["hw"]), what + ", dense prior")
    assert np.isfinite(dense[:nb, D:D + 2, :D + 1]).all() and np.isfinite(dense[:nb][:, c["tri"]]).all()
    table = run(c["Jw_table"], c["hw_table"], c["label"])
    S.same_bits(table, S.assemble_ref(c, c["Jw_expanded"], c["hw_expanded"]), what + ", label / table prior")
    S.same_bits(table, run(c["Jw_expanded"], c["hw_expanded"], None), what + ": the tables against the dense prior they expand to")


# ================================================================================================================ E. pgl_scaled_gram
@pytest.mark.parametrize("D", S.SCALED_D)
@pytest.mark.parametrize("nz", S.SCALED_NZ)
def test_scaled_gram(nz, D):
    """one multiply per element: bit-equal to NumPy on row r, columns 0 .. r | 1 of every slot; rows >= D, the rest of each row and slot nz keep
    their bits; G0 is NaN outside what is read, inv_eta past nz"""
    import torch
    c = S.scaled_gram_case(D, nz)
    G0, inv_eta = _dev(c["G0"]), _dev(c["inv_eta"])
    ref, written = _dev(c["ref"]), _dev(c["written"])
    before = S.poisoned_buffer(ref, torch.zeros_like(written), nz + 1, c["rows"], c["ldj"])
    J = before.clone()
    _call("pgl_scaled_gram", G0=_ptr(G0), ldg=c["ldg"], inv_eta=_ptr(inv_eta), J=_ptr(J), ldj=c["ldj"], strideJ=c["rows"] * c["ldj"], D=D, nz=nz)
    S.check_output(J, before, ref, None, written, "scaled Gram D = %d nz = %d" % (D, nz))
    assert bool(torch.isfinite(J[:nz, :D, :D + 1][written]).all())
