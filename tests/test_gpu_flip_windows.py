"""The proposal windows of the collapsed flips on their own: pgl_flip_decide (decide_kernel<BT> of pgl_flips.hip) and pgl_flip_apply_window
through FlipState, window by window, against the longdouble proposal loop of tests/_dense_ref.py (flip_proposals; held to its definition
on the CPU by tests/test_dense_ref_host.py).

Cases (tests/_flip_window_cases.py): B = 1 ... 8 -- every compiled instantiation --, B = 11 (run-time B, R B odd: the trailing update starts
one row inside the dead window), B = 16 (run-time B, R B even) and B = 32 (R cut by the LDS cap); R = pgl_flip_window_blocks(B) and
N = 2 R + 3: two full windows and a ragged third of 3 blocks, a tableau of about 650 rows.  Four neurons per batch: mixed (flips both ways in
every window, four entries with rho exactly 0 or 1), skipped, nothing flips, everything flips (panels of up to R B = 320 rows).  Each case
runs in both layouts from the same inputs: visit_order = 1 with the tableau uploaded in position order (production) and visit_order = 0 in
J's order.  The device gets the longdouble initial tableau rounded to fp64, so it answers for the windows only.

Conventions of tests/test_gpu_tableau.py: NaN above the diagonal, a sentinel in the padding, NaN scratch, sentinels in d_idx / d_sign /
d_cnt / batch_k and NaN in G before every pgl_flip_decide, a log-odds pre-fill that is neither NaN nor plausible.

Tolerances: decisions, pivot lists, signs, counts and everything said to be untouched are exact.  Log-odds: rtol 1e-10, atol 1e-9 (the
suite's tolerance for this quantity, tests/test_gpu_parity.py).  Tableau and G: max |dev - ref| / max |ref| <= the sum over the windows so
far of 8 Md 2^-53 kappa_2(the window's pivot block as it stood before the window, from the reference).  Every case prints a FLIPWIN line.

Reference time on the host (one core, measured), per case: B = 1: 8.0 s, 2: 6.1 s, 3: 5.5 s, 4: 5.7 s, 5: 6.5 s, 6: 6.0 s, 7: 5.9 s, 8: 6.2 s,
11: 6.2 s, 16: 7.4 s, 32: 2.3 s -- 66 s in all, of which the initial sweep that a case's neurons share is about a fifth.  The B = 8 and
B = 11 cases are built a second time for the tests that use one case only.  The device part of every test takes well under a second."""
import ctypes

import numpy as np
import pytest

from tests import _dense_ref as R
from tests import _flip_window_cases as C

pytestmark = pytest.mark.gpu

SENT = -777.25          # padding of the tableau, d_sign
LO_FILL = -4242.5       # log-odds nobody has written
I_SENT = -9             # d_idx, d_cnt, batch_k
KMAX = 512
LAYOUTS = [1, 0]        # visit_order


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _ldj(N, B):
    from pyglm_amd._lib import call
    v = ctypes.c_int()
    call("pgl_sweep_dims", N, B, 1, None, None, ctypes.byref(v))
    return v.value


def _pack(tabs, Md, ldj):
    """tableaux (Md x Md) -> (nb, ldj, ldj) fp64: the lower triangle, NaN above it, a sentinel in the padding rows and columns"""
    out = np.full((len(tabs), ldj, ldj), SENT)
    il, iu = np.tril_indices(Md), np.triu_indices(Md, 1)
    for n, A in enumerate(tabs):
        out[n][il] = np.asarray(A, dtype=np.float64)[il]
        out[n][iu] = np.nan
    return out


class _Dev:
    """the buffers of one batch on the device and the FlipState over them; neurons: dicts with perm, u, rho, c0, skip"""

    def __init__(self, case, neurons, visit_order, tabs=None):
        import torch
        from pyglm_amd._lib import FlipState
        self.torch = torch
        dev = torch.device("cuda:0")
        N, B, Md = case["N"], case["B"], case["Md"]
        nb, ldj = len(neurons), _ldj(N, B)
        assert ldj >= Md and ldj % 2 == 0
        self.nb, self.ldj = nb, ldj
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        if tabs is None:
            tabs = [R.position_order(case["M0"], nr["perm"], B) if visit_order else case["M0"] for nr in neurons]
        self.Mh = _pack(tabs, Md, ldj)
        up = lambda key, dt: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(nr[key]) for nr in neurons]), dtype=dt)).to(dev)
        self.M = torch.from_numpy(self.Mh).to(dev)
        self.perm, self.u, self.rho, self.c0 = up("perm", np.int32), up("u", np.float64), up("rho", np.float64), up("c0", np.float64)
        self.a = torch.from_numpy(np.tile(np.asarray(case["a0"], dtype=np.int32), (nb, 1))).to(dev)
        self.skip = torch.tensor([int(nr["skip"]) for nr in neurons], **i32)
        self.G = torch.full((nb, KMAX, KMAX), float("nan"), **f64)
        self.Lws = torch.full((nb, (KMAX + 1) ** 2), float("nan"), **f64)
        self.Ut, self.Wt = torch.full((nb, KMAX, ldj), float("nan"), **f64), torch.full((nb, KMAX, ldj), float("nan"), **f64)
        self.status = torch.zeros(nb, **i32)
        self.d_idx, self.d_sign = torch.full((nb, KMAX), I_SENT, **i32), torch.full((nb, KMAX), SENT, **f64)
        self.d_cnt, self.batch_k = torch.full((nb,), I_SENT, **i32), torch.full((nb,), I_SENT, **i32)
        self.logodds = torch.full((nb, N), LO_FILL, **f64)
        self.fields = dict(M=self.M.data_ptr(), ldj=ldj, strideM=ldj * ldj, nb=nb, N=N, B=B, perm=self.perm.data_ptr(), u=self.u.data_ptr(),
                           rho=self.rho.data_ptr(), c0=self.c0.data_ptr(), a=self.a.data_ptr(), skip=self.skip.data_ptr(),
                           d_idx=self.d_idx.data_ptr(), d_sign=self.d_sign.data_ptr(), d_cnt=self.d_cnt.data_ptr(),
                           batch_k=self.batch_k.data_ptr(), G=self.G.data_ptr(), Lws=self.Lws.data_ptr(), Ut=self.Ut.data_ptr(),
                           Wt=self.Wt.data_ptr(), ldu=ldj, status=self.status.data_ptr(), visit_order=visit_order,
                           logodds=self.logodds.data_ptr())
        self.s = FlipState(**self.fields)

    def refill(self):
        self.d_idx.fill_(I_SENT); self.d_sign.fill_(SENT); self.d_cnt.fill_(I_SENT); self.batch_k.fill_(I_SENT); self.G.fill_(float("nan"))

    def snap(self, with_G):
        self.torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in ("M", "a", "logodds", "d_idx", "d_sign", "d_cnt", "batch_k", "status")}
        if with_G:
            out["G"] = self.G.cpu().numpy()
        return out

    def decide(self, w):
        from pyglm_amd._lib import call
        self.refill()
        call("pgl_flip_decide", ctypes.byref(self.s), w, None)
        return self.snap(True)

    def apply(self, w):
        from pyglm_amd._lib import call
        call("pgl_flip_apply_window", ctypes.byref(self.s), w, None)
        return self.snap(False)

    def windows(self, ws):
        return [(self.decide(w), self.apply(w)) for w in ws]


def _neurons(case, kinds=C.KINDS):
    return [case["neurons"][k] for k in kinds]


def _batch(case, vo):
    """the four neurons of the case through all windows in layout vo -> (host copy of the uploaded tableaux, [(after decide, after apply)])"""
    if vo not in case["_runs"]:
        d = _Dev(case, _neurons(case), vo)
        case["_runs"][vo] = (d.Mh, d.windows(range(case["nwin"])))
    return case["_runs"][vo]


@pytest.fixture(scope="module", params=C.BLOCK_SIZES, ids=lambda b: "B%d" % b)
def case(request):
    """inputs and references of one block size (the input conditions are asserted while it is built, before anything runs on the device);
    the device results of its two layouts are kept beside it and go with it"""
    c = C.build_case(request.param)
    c["_runs"] = {}
    yield c
    c["_runs"].clear()


def _same_state(x, y, what):
    for k in x:
        assert np.array_equal(_bits(x[k]) if x[k].dtype == np.float64 else x[k], _bits(y[k]) if y[k].dtype == np.float64 else y[k]), \
            "%s: %s differs" % (what, k)


# ---------------------------------------------------------------------------------------------------------------- every case, both layouts
@pytest.mark.parametrize("vo", LAYOUTS, ids=lambda v: "visit_order%d" % v)
def test_windows_against_reference(case, vo):
    B, Rw, N, D, Md, nwin = (case[k] for k in ("B", "R", "N", "D", "Md", "nwin"))
    Mh, steps = _batch(case, vo)
    worst_m = worst_g = worst_lo = worst_ratio = 0.0
    last_bound = 0.0
    for n, kind in enumerate(C.KINDS):
        nr = case["neurons"][kind]
        ref, perm = nr["ref"], nr["perm"]
        M_prev, lo_prev, bnd = Mh[n], np.full(N, LO_FILL), 0.0
        for w, (dec, app) in enumerate(steps):
            tag = "B = %d visit_order = %d %s window %d" % (B, vo, kind, w)
            k_lo, k_hi = w * Rw, min((w + 1) * Rw, N)
            # ---- after pgl_flip_decide(w)
            assert dec["status"][n] == 0 and app["status"][n] == 0, tag
            assert np.array_equal(_bits(dec["M"][n]), _bits(M_prev)), tag + ": the proposals wrote to the tableau"
            lo = dec["logodds"][n]
            if kind == "skipped":
                assert dec["d_cnt"][n] == 0 and dec["batch_k"][n] == 0, tag
                assert np.array_equal(dec["a"][n], case["a0"].astype(np.int32)) and np.all(lo == LO_FILL), tag
                assert np.all(dec["d_idx"][n] == I_SENT) and np.all(dec["d_sign"][n] == SENT), tag
                assert np.array_equal(_bits(app["M"][n]), _bits(M_prev)), tag + ": a skipped neuron's tableau was touched"
                continue
            flips = ref["win_flips"][w]
            cnt = B * len(flips)
            Mref, aref = ref["snaps"][w]
            assert np.array_equal(dec["a"][n], aref.astype(np.int32)), tag + ": decisions"
            assert np.array_equal(_bits(lo[:k_lo]), _bits(lo_prev[:k_lo])) and np.all(lo[k_hi:] == LO_FILL), tag + ": log-odds of other windows"
            want = ref["logodds"][k_lo:k_hi].astype(np.float64)
            got = lo[k_lo:k_hi]
            assert np.array_equal(np.isnan(got), np.isnan(want)), tag + ": NaN log-odds exactly where rho is 0 or 1"
            assert np.isnan(want).sum() == sum(1 for k in ref["special"] if k_lo <= k < k_hi)
            ok = ~np.isnan(want)
            np.testing.assert_allclose(got[ok], want[ok], rtol=1e-10, atol=1e-9, err_msg=tag)
            worst_lo = max(worst_lo, float(np.max(np.abs(got[ok] - want[ok]))))
            assert dec["d_cnt"][n] == cnt and dec["batch_k"][n] == (cnt + 15) & ~15, tag
            rows_j = np.array([m * B + b for _, m, _ in flips for b in range(B)], dtype=int)
            rows_dev = np.array([(k if vo else m) * B + b for k, m, _ in flips for b in range(B)], dtype=int)
            sg = np.repeat([float(s) for _, _, s in flips], B)
            assert np.array_equal(dec["d_idx"][n][:cnt], rows_dev) and np.all(dec["d_idx"][n][cnt:] == I_SENT), tag + ": d_idx"
            assert np.array_equal(dec["d_sign"][n][:cnt], sg) and np.all(dec["d_sign"][n][cnt:] == SENT), tag + ": d_sign"
            bnd += 8.0 * Md * R.U53 * ref["kappa"][w]
            G, bk = dec["G"][n], (cnt + 15) & ~15
            if cnt:
                Gref = -(R.ld(sg)[:, None] * R.ld(sg)[None, :]) * Mref[np.ix_(rows_j, rows_j)]
                eg = R.relerr(G[:cnt, :cnt], Gref)
                worst_g, worst_ratio = max(worst_g, eg), max(worst_ratio, eg / bnd)
                assert eg <= bnd, tag + ": G %.2e > bound %.2e" % (eg, bnd)
            around = G[:bk].copy()
            around[:cnt, :cnt] = 0.0
            assert not around.any(), tag + ": G is not exactly zero around its corner"
            # ---- after pgl_flip_apply_window(w)
            got = app["M"][n]
            for k in ("a", "logodds", "d_idx", "d_sign", "d_cnt", "batch_k"):
                assert np.array_equal(app[k][n], dec[k][n], equal_nan=True), tag + ": the update wrote to " + k
            if vo == 0:
                il = np.tril_indices(Md)
                em = R.relerr(got[:Md, :Md][il], Mref[il])
                assert np.all(got[Md:, :] == SENT) and np.all(got[:, Md:] == SENT), tag + ": padding"
            elif w == nwin - 1 or cnt == 0:
                assert np.array_equal(_bits(got), _bits(M_prev)), tag + ": nothing may be written"
                em = 0.0
            else:
                p1 = (w + 1) * Rw * B
                r0 = p1 & ~1
                il = np.tril_indices(Md - p1)
                em = R.relerr(got[p1:Md, p1:Md][il], R.position_order(Mref, perm, B)[p1:, p1:][il])
                dead = np.ones(got.shape, dtype=bool)
                dead[r0:, r0:] = False
                assert np.array_equal(_bits(got)[dead], _bits(M_prev)[dead]), tag + ": a write outside the trailing square"
                assert np.all(got[Md:, :] == SENT) and np.all(got[:, Md:] == SENT), tag + ": padding"
            if kind == "nothing":
                assert np.array_equal(_bits(got), _bits(M_prev)), tag + ": no flip, but the tableau changed"
            worst_m = max(worst_m, em)
            if bnd > 0:
                worst_ratio = max(worst_ratio, em / bnd)
            assert em <= bnd, tag + ": tableau %.2e > bound %.2e" % (em, bnd)
            M_prev, lo_prev, last_bound = got, lo, max(last_bound, bnd)
    print("FLIPWIN B=%d R=%d N=%d visit_order=%d  tableau err %.2e  G err %.2e  bound (all windows) %.2e  largest err/bound %.3g  log-odds diff %.2e"
          % (B, Rw, N, vo, worst_m, worst_g, last_bound, worst_ratio, worst_lo))


# ---------------------------------------------------------------------------------------------------------------- one case each
@pytest.mark.parametrize("case", [8, 11], indirect=True, ids=lambda b: "B%d" % b)
def test_a_neuron_alone_gives_the_bits_it_gives_in_the_batch(case):
    _, steps = _batch(case, 1)
    for kind in ("mixed", "everything"):
        n = C.KINDS.index(kind)
        alone = _Dev(case, _neurons(case, [kind]), 1).windows(range(case["nwin"]))
        for w, (both, one) in enumerate(zip(steps, alone)):
            for i in (0, 1):
                _same_state({k: v[n] for k, v in both[i].items()}, {k: v[0] for k, v in one[i].items()},
                            "%s alone, window %d, after %s" % (kind, w, ("decide", "apply")[i]))


@pytest.mark.parametrize("case", [8], indirect=True, ids=lambda b: "B%d" % b)
@pytest.mark.parametrize("vo", LAYOUTS, ids=lambda v: "visit_order%d" % v)
def test_a_window_past_the_last_proposes_nothing(case, vo):
    d = _Dev(case, _neurons(case), vo)
    before = d.snap(True)
    dec, app = d.windows([case["nwin"]])[0]
    assert np.all(dec["d_cnt"] == 0) and np.all(dec["batch_k"] == 0) and np.all(app["d_cnt"] == 0) and np.all(app["batch_k"] == 0)
    for after in (dec, app):
        _same_state({k: before[k] for k in ("M", "a", "logodds", "d_idx", "d_sign", "status")}, {k: after[k] for k in ("M", "a", "logodds", "d_idx", "d_sign", "status")},
                    "window %d of %d" % (case["nwin"], case["nwin"]))


@pytest.mark.parametrize("case", [8], indirect=True, ids=lambda b: "B%d" % b)
def test_a_block_that_is_not_positive_definite_is_flagged_on_its_neuron_only(case):
    """a fifth neuron, the mixed one again, with the diagonal block of an inactive block of window 0 negated in the uploaded tableau: status
    bit 1 on that neuron, every other neuron's outputs the same bits as without it"""
    B = case["B"]
    _, steps = _batch(case, 1)
    mixed = case["neurons"]["mixed"]
    k = next(k for k in range(case["R"]) if not case["a0"][mixed["perm"][k]] and k not in mixed["ref"]["special"])
    neurons = _neurons(case) + [mixed]
    tabs = [R.position_order(case["M0"], nr["perm"], B).copy() for nr in neurons]
    tabs[4][k * B:(k + 1) * B, k * B:(k + 1) * B] *= -1.0
    dec, app = _Dev(case, neurons, 1, tabs=tabs).windows([0])[0]
    assert dec["status"][4] & 1 and app["status"][4] & 1
    assert not dec["status"][:4].any() and not app["status"][:4].any()
    for i, got in enumerate((dec, app)):
        _same_state({k: v[:4] for k, v in steps[0][i].items()}, {k: v[:4] for k, v in got.items()}, "beside a flagged neuron, after %s" % ("decide", "apply")[i])


@pytest.mark.parametrize("case", [8], indirect=True, ids=lambda b: "B%d" % b)
def test_the_production_chain_from_J(case):
    """pgl_flip_visit_order from J's tableau, pgl_flip_apply_chunk on the host-built list (bias first, then the active positions ascending),
    then the three windows, visit_order = 1: the reference's decisions, its log-odds within the tolerance"""
    import torch
    from pyglm_amd._lib import call
    B, N, D, Md = (case[k] for k in ("B", "N", "D", "Md"))
    neurons = _neurons(case)
    d = _Dev(case, neurons, 1, tabs=[np.full((Md, Md), SENT)] * len(neurons))
    src = torch.from_numpy(_pack([R.tableau(case["J"], case["h"])] * d.nb, Md, d.ldj)).to(d.M.device)
    d.M.fill_(SENT)
    call("pgl_flip_visit_order", ctypes.byref(d.s), ctypes.c_void_p(src.data_ptr()), d.ldj, d.ldj * d.ldj, None)
    ih, ch = np.zeros((d.nb, KMAX), dtype=np.int32), np.zeros(d.nb, dtype=np.int32)
    for n, nr in enumerate(neurons):
        if nr["skip"]:
            continue
        lst = [D] + [k * B + b for k in range(N) if case["a0"][nr["perm"][k]] for b in range(B)]
        assert len(lst) <= KMAX
        ih[n, :len(lst)], ch[n] = lst, len(lst)
    d.d_idx.copy_(torch.from_numpy(ih)); d.d_sign.fill_(1.0); d.d_cnt.copy_(torch.from_numpy(ch))
    call("pgl_flip_apply_chunk", ctypes.byref(d.s), KMAX, None)
    torch.cuda.synchronize()
    assert not d.status.cpu().numpy().any()
    worst = 0.0
    for w in range(case["nwin"]):
        dec, _ = d.decide(w), d.apply(w)
        for n, kind in enumerate(C.KINDS):
            ref = case["neurons"][kind]["ref"]
            assert dec["status"][n] == 0
            if ref is None:
                assert dec["d_cnt"][n] == 0 and np.array_equal(dec["a"][n], case["a0"].astype(np.int32))
                continue
            assert np.array_equal(dec["a"][n], ref["snaps"][w][1].astype(np.int32)), "%s window %d" % (kind, w)
            assert dec["d_cnt"][n] == B * len(ref["win_flips"][w])
    lo = d.logodds.cpu().numpy()
    for n, kind in enumerate(C.KINDS):
        ref = case["neurons"][kind]["ref"]
        if ref is None:
            assert np.all(lo[n] == LO_FILL)
            continue
        want = ref["logodds"].astype(np.float64)
        assert np.array_equal(np.isnan(lo[n]), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_allclose(lo[n][ok], want[ok], rtol=1e-10, atol=1e-9, err_msg=kind)
        worst = max(worst, float(np.max(np.abs(lo[n][ok] - want[ok]))))
    print("FLIPWIN production chain B=%d  log-odds diff %.2e" % (B, worst))


@pytest.mark.parametrize("case", [8], indirect=True, ids=lambda b: "B%d" % b)
def test_decide_refuses_what_its_kernel_would_write_through(case):
    """G and batch_k are written unconditionally, one workgroup per neuron, the tableau is read at ldj: a state without them is refused before
    anything is launched"""
    from pyglm_amd._lib import FlipState, PglError, call
    d = _Dev(case, _neurons(case), 1)
    before = d.snap(True)
    for bad in (dict(G=None), dict(batch_k=None), dict(nb=0), dict(ldj=case["Md"] - 1)):
        s = FlipState(**dict(d.fields, **bad))
        with pytest.raises(PglError):
            call("pgl_flip_decide", ctypes.byref(s), 0, None)
    after = d.snap(True)
    _same_state(before, after, "after the refused calls")
    assert np.all(after["d_cnt"] == I_SENT) and np.all(after["logodds"] == LO_FILL)
