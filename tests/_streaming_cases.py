"""Cases, inputs and references of tests/test_gpu_streaming.py, built with NumPy alone (tests/test_streaming_cases_host.py checks them without a
GPU).  The streaming kernels of pgl_elementwise.hip and the shared walk over Psi of pgl_obs.h, entry point by entry point.

The launch geometry is RESTATED here -- the tests choose their shapes from it:
    walk over Psi   one block per PGLL_ROWS = 64 time bins; narrow walk where nloc < 64 and obs != 2 (one column group), else lane = neuron in
                    64-column groups.  Wave w of a block adds rows w, w + 4, ... of the block, the four sums combine as ((r0 + r1) + r2) + r3,
                    the blocks' partials are added ascending, then out (+)= s (emulate_reduction)
    assembly        256-column chunks over the D + 1 columns 0 .. D of a neuron
    transpose       32 x 32 tiles
    convolution     256 cells (t, n) per block, t = idx / N, n = idx % N; the basis [R][B] in dynamic LDS (above 64 KiB the limit is raised, above
                    160 KiB the call is refused)
    scaled Gram     row r < D, thread pairs c = 0, 2, ... with c <= r and c < D: columns 0 .. r | 1 of every slot (scaled_gram_written)

Two kinds of operands for the convolution, as in tests/_contraction_cases.py.
  "exact"  S counts in 0 .. 3, basis entries k / 1024 with |k| <= 1024: every product and partial sum is an integer multiple of 2^-10 below
           R * 3 <= 2^10, so every order of addition and every fma contraction gives the same fp64 bits (conv_exact_premise proves it in int64).
  "real"   element-wise within (R + 2) 2^-53 sum_l |basis[l][b]| |S[t-1-l][n]|: the any-order bound of a length-R fp64 dot product.
The Gaussian pass of section C has residuals r with 24-bit significands (float32 values): r * r is an exact fp64 number, so a compiler that
contracts `ll += r * r` into one fma and one that does not add the same terms; the sums themselves still round, so their order shows.

Poison: whatever a kernel must not write, and whatever it must not read into a stored value, is NaN; buffers are compared as int64 bit patterns
(same_bits).  poisoned_buffer and check_output of tests/_contraction_cases.py serve where the layout is theirs ([slots][rows][ld])."""
import math

import numpy as np

from tests._contraction_cases import check_output, poisoned_buffer  # noqa: F401  (re-exported for the GPU tests)

U = 2.0 ** -53
LD = np.longdouble
PGLL_ROWS = 64
PGL_ERR_ARG = 1                     # pgl_common.h
LDS_DEFAULT, LDS_MAX = 64 * 1024, 160 * 1024


# ------------------------------------------------------------------------------------------------------------ the geometry, restated
def psi_narrow(nloc, obs):
    return nloc < 64 and obs != 2


def psi_row_blocks(T):
    return -(-T // PGLL_ROWS)


def conv_blocks(T, N):
    return -(-(T * N) // 256)


def conv_lds_bytes(R, B):
    return R * B * 8


def assembly_chunks(N, B):
    return -(-(N * B + 1) // 256)


def transpose_tiles(rows, cols):
    return -(-rows // 32), -(-cols // 32)


def pg_stream(sweep, neuron):
    """the stream of neuron `neuron` (global index) in sweep `sweep`"""
    return (sweep << 32) | (neuron & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------ poison and guards
# A SIGNALING NaN: arithmetic on it returns a quiet NaN, other bits -- a kernel that adds to a guarded cell changes it, where a quiet NaN would
# come back as it was.  Copies keep the bits.
SNAN_BITS = 0x7FF0000000000001


def guarded(values, rows, ld, fill=np.nan):
    """[rows][ld] of `fill` with the 2-D `values` in its top left corner"""
    buf = np.full((rows, ld), fill, dtype=np.float64)
    buf[:values.shape[0], :values.shape[1]] = values
    return buf


def guarded_vec(values, n):
    buf = np.full(n, np.nan)
    buf[:len(values)] = values
    return buf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(got, expect, what=""):
    """every element the same bit pattern (NaN payloads and the sign of zero included)"""
    got, expect = np.asarray(got), np.asarray(expect)
    assert got.shape == expect.shape, "%s: shapes %s and %s" % (what, got.shape, expect.shape)
    bad = bits(got) != bits(expect)
    assert not bad.any(), "%s: %d of %d elements differ in bits, first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


# ================================================================================================================ A. pgl_design_matrix
DESIGN_SHAPES = [(1, 1, 1, 1), (5, 3, 2, 9), (37, 7, 3, 4), (300, 1, 32, 3), (65, 4, 1, 1), (40, 5, 8, 40)]     # (T, N, B, R)
DESIGN_LDS_SHAPE = (300, 2, 32, 257)            # R * B * 8 = 65 792 bytes: just past the 64 KiB a launch gets without the limit raised
DESIGN_LDS_REFUSED = (4, 1, 32, 641)            # R * B * 8 = 164 096 bytes > 160 KiB
KINDS = ["exact", "real"]


def design_case(kind, T, N, B, R, seed=0):
    """S [T + 2][lds] with NaN in the padding columns and the rows past T, basis [R][B] with negative entries; X [T + 2][ldx] and Xt [D + 3][ldxt]
    are NaN on entry.  lds > N, ldx > N B + 1, ldxt > T."""
    rng = np.random.default_rng(1000 * T + 100 * N + 10 * B + R + seed)
    if kind == "exact":
        S = rng.integers(0, 4, (T, N)).astype(np.float64) * (rng.random((T, N)) < 0.6)
        basis = rng.integers(-1024, 1025, (R, B)).astype(np.float64) / 1024
    else:
        S = rng.standard_normal((T, N)) * (rng.random((T, N)) < 0.6)
        basis = rng.standard_normal((R, B))
    D = N * B
    c = dict(kind=kind, T=T, N=N, B=B, R=R, D=D, lds=N + 3, ldx=D + 4, ldxt=T + 5, x_rows=T + 2, xt_rows=D + 3, S=S, basis=basis)
    c["S_buf"] = guarded(S, T + 2, c["lds"])
    return c


def design_ref(S, basis, clip):
    """(X [T][D + 1] in longdouble, mag [T][D + 1]): X[t][n B + b] = sum_l basis[l][b] S[t - 1 - l][n] (clipped at 0), the ones column at D;
    mag the same sum of magnitudes (0 in the ones column)"""
    T, N = S.shape
    R, B = basis.shape
    X, mag = np.zeros((T, N, B), dtype=LD), np.zeros((T, N, B))
    Sl, bl = S.astype(LD), basis.astype(LD)
    for l in range(min(R, T - 1)):
        X[l + 1:] += Sl[:T - 1 - l, :, None] * bl[l][None, None, :]
        mag[l + 1:] += np.abs(S[:T - 1 - l, :, None]) * np.abs(basis[l])[None, None, :]
    if clip:
        X = np.maximum(X, 0)
    ones = np.ones((T, 1))
    return np.concatenate([X.reshape(T, N * B), ones.astype(LD)], axis=1), np.concatenate([mag.reshape(T, N * B), 0 * ones], axis=1)


def design_bound(mag, R):
    return (R + 2) * U * mag


def conv_exact_premise(S, basis):
    """the premise of the exact cases: S and 1024 basis are integers, and the largest magnitude a partial sum can reach, in units of 2^-10, is
    returned (below 2^53 every partial sum of every order is an exact fp64 number)"""
    Si, bi = np.rint(S).astype(np.int64), np.rint(basis * 1024).astype(np.int64)
    assert np.array_equal(Si, S) and np.array_equal(bi / 1024.0, basis) and Si.min() >= 0 and Si.max() <= 3 and np.abs(bi).max() <= 1024
    return int(np.abs(Si).max(initial=0)) * int(np.abs(bi).sum(axis=0).max())


def history_blocks(T, R):
    """(r0, r1) row blocks of the block-with-history call: one that starts inside the first R rows (h = r0 < R, where T allows) and one with a
    full history (h = R), each ending before or at T"""
    out = [(r0, r1) for r0, r1 in ((min(R, T) // 2, T), (R + 1, T), (R, min(T, R + 3)), (0, min(T, 2))) if 0 <= r0 < r1 <= T]
    return sorted(set(out))


# ================================================================================================================ B. pgl_transpose
TRANSPOSE_SHAPES = [(r, c) for r in (1, 31, 32, 33, 65) for c in (1, 32, 33, 70)]


def transpose_case(rows, cols):
    """src [rows + 2][cols + 3] NaN outside [:rows, :cols] (some -0.0 and a subnormal inside), dst [cols + 2][rows + 5] NaN on entry"""
    rng = np.random.default_rng(100 * rows + cols)
    v = rng.standard_normal((rows, cols))
    v[rng.random((rows, cols)) < 0.1] = -0.0
    v[0, 0] = 5e-324
    return dict(rows=rows, cols=cols, ld_src=cols + 3, ld_dst=rows + 5, values=v, src=guarded(v, rows + 2, cols + 3), dst=np.full((cols + 2, rows + 5), np.nan))


# ================================================================================================================ C. the pass over Psi
PSI_T = [1, 63, 64, 65, 130, 257]
PSI_NLOC = [1, 5, 63, 64, 65, 130]
# every T edge with a narrow (5) and a wide (65) column count, every nloc edge with T = 130
PSI_SHAPES = sorted(set([(T, n) for T in PSI_T for n in (5, 65)] + [(130, n) for n in PSI_NLOC]))
PSI_PRODUCTION = [(65, 5), (130, 130)]                       # the shapes that run in the production layout [Omega | Kappa]
# variant -> (obs, per-neuron param)
PSI_VARIANTS = {"bernoulli": (0, False), "negbin": (1, False), "negbin_param": (1, True), "binomial": (3, False), "binomial_param": (3, True),
                "hooks": (4, False)}
GAUSS_SHAPES = [(T, n) for T in PSI_T for n in (5, 65)]
SEED, SWEEP, NEURON0, ELEM0 = 0x1234ABCD5678, 3, 1000, 77777      # all nonzero: a kernel that drops one of them draws other numbers
XI0, NBIN0 = 2.5, 12.0


def _round_up(x, m):
    return -(-x // m) * m


def psi_case(T, nloc, variant, layout=None, seed=0):
    """One pass: Psi [T + 1][ldpsi], bias, Y [T + 1][ldy], param, hooks [T][3 ldh] with NaN in every padding column and guard row, |psi + bias| <= 30.
    layout "production": Omega and Kappa halves of one [Tp + 1][2 ldn] array, Tp = ceil(T / 16) 16; else unrelated leading dimensions.
    a, b, logc_known ([T][nloc]): the cell's terms as the kernel forms them (b = y + xi is one fp64 addition)."""
    obs, per_neuron = PSI_VARIANTS[variant]
    if layout is None:
        layout = "production" if (T, nloc) in PSI_PRODUCTION else "unrelated"
    rng = np.random.default_rng(100000 * obs + 1000 * T + 7 * nloc + per_neuron + seed)
    psi = rng.uniform(-26.0, 26.0, (T, nloc))
    psi[rng.random((T, nloc)) < 0.5] /= 8                   # half of the cells where neither tail of log1p(exp) is flat
    bias = rng.uniform(-4.0, 4.0, nloc)
    c = dict(T=T, nloc=nloc, variant=variant, obs=obs, layout=layout, ldpsi=nloc + 3, ldy=nloc + 5, ldh=nloc + 4, xi=0.0, param=None, hooks=None)
    rate = 1.0 / (1.0 + np.exp(-(psi + bias) / 8))
    if obs == 0 or obs == 4:
        Y = (rng.random((T, nloc)) < rate).astype(np.float64)
    if obs == 1:
        Y = rng.poisson(3.0 * rate).astype(np.float64)
        xi = rng.uniform(0.3, 6.0, nloc) if per_neuron else np.full(nloc, XI0)
        c.update(xi=XI0, param=xi if per_neuron else None, p=xi)
        a, b = Y, Y + xi[None, :]
    elif obs == 3:
        m = rng.integers(1, 21, nloc).astype(np.float64) if per_neuron else np.full(nloc, NBIN0)
        Y = rng.binomial(m.astype(np.int64)[None, :], rate).astype(np.float64)
        c.update(xi=NBIN0, param=m if per_neuron else None, p=m)
        a, b = Y, np.broadcast_to(m, (T, nloc)).copy()
    elif obs == 4:
        a, b, logc = rng.uniform(-2.0, 5.0, (T, nloc)), rng.uniform(0.25, 6.0, (T, nloc)), rng.uniform(-3.0, 3.0, (T, nloc))
        hooks = np.full((T, 3 * c["ldh"]), np.nan)
        for k, v in enumerate((a, b, logc)):
            hooks[:, k * c["ldh"]:k * c["ldh"] + nloc] = v
        c.update(hooks=hooks, logc=logc)
    else:
        a, b = Y, np.ones((T, nloc))
    c.update(psi=psi, bias=bias, Y=Y, a=a, b=b, Psi_buf=guarded(psi, T + 1, c["ldpsi"]), Y_buf=guarded(Y, T + 1, c["ldy"]),
             bias_buf=guarded_vec(bias, nloc + 2), param_buf=None if c["param"] is None else guarded_vec(c["param"], nloc + 2))
    if layout == "production":
        ldn = _round_up(nloc, 2) + 2
        c.update(ldn=ldn, ldo=2 * ldn, ldk=2 * ldn, ok_rows=_round_up(T, 16) + 1)
    else:
        c.update(ldo=nloc + 7, ldk=nloc + 2, ok_rows=T + 1)
    return c


def hooks_of_bernoulli(c):
    """the hooks (y, 1, 0) of a Bernoulli case: [T][3 ldh], NaN in the padding"""
    T, nloc, ldh = c["T"], c["nloc"], c["ldh"]
    hooks = np.full((T, 3 * ldh), np.nan)
    hooks[:, :nloc], hooks[:, ldh:ldh + nloc], hooks[:, 2 * ldh:2 * ldh + nloc] = c["Y"], 1.0, 0.0
    return hooks


def _lgamma(x):
    return np.vectorize(math.lgamma, otypes=[np.float64])(x)


def ll_reference(c, psi_out):
    """(l [T][nloc] in longdouble, cap [T][nloc]): the cell's term log c + a psi - b log1p(exp psi) with log c formed WITHOUT lgamma -- negative
    binomial sum_{k < y} log((xi + k) / (k + 1)), binomial the log of the exact integer coefficient --, and the cap on the fp64 error,
    16 2^-53 (|lgamma| of the three arguments + |a psi| + b log1p(exp psi)); hooks: |log c| where the lgammas stand (log c is an input there)"""
    obs, Y, a, b = c["obs"], c["Y"], c["a"].astype(LD), c["b"].astype(LD)
    T, nloc = Y.shape
    psi = psi_out.astype(LD)
    logc, lg = np.zeros((T, nloc), dtype=LD), np.zeros((T, nloc))
    if obs == 1:
        p = np.broadcast_to(c["p"], (T, nloc))
        for k in range(int(Y.max(initial=0))):
            logc += np.where(Y > k, np.log((p.astype(LD) + k) / (k + 1)), 0)
        lg = np.abs(_lgamma(Y + p)) + np.abs(_lgamma(Y + 1)) + np.abs(_lgamma(p))
    elif obs == 3:
        m = np.broadcast_to(c["p"], (T, nloc))
        comb = np.vectorize(lambda n, y: LD(math.comb(int(n), int(y))), otypes=[LD])(m, Y)
        logc = np.log(comb)
        lg = np.abs(_lgamma(m + 1)) + np.abs(_lgamma(Y + 1)) + np.abs(_lgamma(m - Y + 1))
    elif obs == 4:
        logc, lg = c["logc"].astype(LD), np.abs(c["logc"])
    soft = np.log1p(np.exp(psi))
    l = logc + a * psi - b * soft
    cap = 16 * U * (lg + np.abs(c["a"] * psi_out) + c["b"] * soft.astype(np.float64))
    return l, cap


def ll_formula_fp64(c, psi_out):
    """the header's formula in NumPy fp64, lgamma and all: what the host test holds under the same cap"""
    obs, Y = c["obs"], c["Y"]
    logc = np.zeros_like(Y)
    if obs == 1:
        logc = _lgamma(Y + c["p"]) - _lgamma(Y + 1.0) - _lgamma(np.broadcast_to(c["p"], Y.shape))
    elif obs == 3:
        logc = _lgamma(c["p"] + 1.0) - _lgamma(Y + 1.0) - _lgamma(c["p"] - Y + 1.0)
    elif obs == 4:
        logc = c["logc"]
    return logc + c["a"] * psi_out - c["b"] * np.log1p(np.exp(psi_out))


def emulate_reduction(terms, out0=None, wave_order=(0, 1, 2, 3)):
    """(out [nloc], partials [blocks][nloc]) of the device's reduction of terms [T][nloc], in fp64: wave w adds rows w, w + 4, ... of a 64-row
    block from 0.0, the four sums combine as ((r0 + r1) + r2) + r3, the blocks are added ascending from 0.0, then out = out0 + s (or s)"""
    terms = np.asarray(terms, dtype=np.float64)
    T, nloc = terms.shape
    nblk = psi_row_blocks(T)
    part = np.zeros((nblk, nloc))
    for blk in range(nblk):
        t0 = blk * PGLL_ROWS
        red = []
        for w in range(4):
            acc = np.zeros(nloc)
            for t in range(t0 + w, min(T, t0 + PGLL_ROWS), 4):
                acc = acc + terms[t]
            red.append(acc)
        o = wave_order
        part[blk] = ((red[o[0]] + red[o[1]]) + red[o[2]]) + red[o[3]]
    s = np.zeros(nloc)
    for blk in range(nblk):
        s = s + part[blk]
    return (s if out0 is None else np.asarray(out0, dtype=np.float64) + s), part


def gauss_case(T, nloc, seed=0):
    """The Gaussian pass: psi and bias multiples of 1 / 16, residuals r float32 values (24-bit significands) over several binades, y = psi + bias
    + r an exact fp64 number: y - (psi + bias) == r and r * r exact in fp64 (gauss_exact_premise)."""
    rng = np.random.default_rng(5000 * T + nloc + seed)
    psi = rng.integers(-256, 257, (T, nloc)) / 16.0
    bias = rng.integers(-64, 65, nloc) / 16.0
    r = (rng.standard_normal((T, nloc)) * 2.0 ** rng.integers(-6, 3, (T, nloc))).astype(np.float32).astype(np.float64)
    r = np.where(np.abs(r) < 2.0 ** -12, 2.0 ** -12, r)     # (lowest bit >= 2^-35: psi + bias + r below is exact)
    Y = (psi + bias) + r
    inv_eta = rng.uniform(0.2, 3.0, nloc)
    c = dict(T=T, nloc=nloc, obs=2, layout="unrelated", psi=psi, bias=bias, Y=Y, r=r, inv_eta=inv_eta, ldpsi=nloc + 3, ldy=nloc + 5, ldo=nloc + 7, ldk=nloc + 2,
             ok_rows=T + 1, Psi_buf=guarded(psi, T + 1, nloc + 3), Y_buf=guarded(Y, T + 1, nloc + 5), bias_buf=guarded_vec(bias, nloc + 2),
             inv_eta_buf=guarded_vec(inv_eta, nloc + 2))
    return c


def gauss_exact_premise(c):
    from fractions import Fraction
    psi_out = c["psi"] + c["bias"]
    assert np.array_equal(c["Y"] - psi_out, c["r"]) and np.array_equal(c["r"].astype(np.float32).astype(np.float64), c["r"])
    sq = c["r"] * c["r"]
    flat_r, flat_sq = c["r"].ravel(), sq.ravel()
    pick = np.random.default_rng(0).integers(0, flat_r.size, min(flat_r.size, 200))
    assert all(Fraction(float(flat_r[i])) ** 2 == Fraction(float(flat_sq[i])) for i in pick)
    return sq


# ================================================================================================================ D. pgl_assemble_posterior
ASSEMBLE_SHAPES = [(51, 5), (64, 4), (257, 1), (8, 32), (1, 1)]      # (N, B): D = 255 and 256 put column D on either side of a chunk edge
ASSEMBLE_NB = [1, 3]
ASSEMBLE_K = 3


def triangle_mask(N, B, rows, ld):
    """[rows][ld] bool: the lower triangles of the B x B diagonal blocks"""
    m = np.zeros((rows, ld), dtype=bool)
    r = np.arange(N * B)
    for bj in range(B):
        rr = r[r % B >= bj]
        m[rr, rr - rr % B + bj] = True
    return m


def assemble_case(N, B, nb, seed=0):
    """J [nb + 1][D + 4][ldj] (signaling) NaN but for the lower triangles of the diagonal blocks of the first nb slots; border sums bo, bk [nb + 1][ldb] with
    NaN beyond column D and in the guard row; the prior dense (Jw [nb][N][B][B], hw [nb][N][B]) and as tables of K = 3 blocks with random labels,
    plus the dense prior the tables expand to."""
    rng = np.random.default_rng(1000 * N + 10 * B + nb + seed)
    D = N * B
    c = dict(N=N, B=B, nb=nb, D=D, rows=D + 4, ldj=D + 5, ldb=D + 3)
    tri = triangle_mask(N, B, c["rows"], c["ldj"])
    J = np.full((nb + 1, c["rows"], c["ldj"]), SNAN_BITS, dtype=np.uint64).view(np.float64)     # (signaling: an addition on a guarded cell shows)
    J[:nb, tri] = rng.standard_normal((nb, int(tri.sum())))
    bo, bk = (guarded(rng.standard_normal((nb, D + 1)), nb + 1, c["ldb"]) for _ in range(2))
    Jw_t, hw_t = rng.standard_normal((ASSEMBLE_K, B, B)), rng.standard_normal((ASSEMBLE_K, B))
    label = rng.integers(0, ASSEMBLE_K, (nb, N)).astype(np.int32)
    c.update(tri=tri, J=J, bo=bo, bk=bk, Jw=rng.standard_normal((nb, N, B, B)), hw=rng.standard_normal((nb, N, B)), Jb=guarded_vec(rng.standard_normal(nb), nb + 1),
             hb=guarded_vec(rng.standard_normal(nb), nb + 1), Jw_table=Jw_t, hw_table=hw_t, label=label, Jw_expanded=Jw_t[label], hw_expanded=hw_t[label])
    return c


def assemble_ref(c, Jw, hw):
    """J after the call, every element: the triangles + Jw, row D = [bo[:D], bo[D] + Jb], row D + 1 = [bk[:D] + hw, bk[D] + hb, 0]; each one
    fp64 addition or a copy.  Everything else as on entry."""
    N, B, nb, D = c["N"], c["B"], c["nb"], c["D"]
    out = c["J"].copy()
    for n in range(nb):
        for m in range(N):
            blk = slice(m * B, (m + 1) * B)
            low = np.tril(np.ones((B, B), dtype=bool))
            sub = out[n, blk, blk]
            sub[low] = sub[low] + Jw[n, m][low]
        out[n, D, :D] = c["bo"][n, :D]
        out[n, D, D] = c["bo"][n, D] + c["Jb"][n]
        out[n, D + 1, :D] = c["bk"][n, :D] + hw[n].reshape(D)
        out[n, D + 1, D] = c["bk"][n, D] + c["hb"][n]
        out[n, D + 1, D + 1] = 0.0
    return out


# ================================================================================================================ E. pgl_scaled_gram
SCALED_D = [1, 2, 3, 16, 17, 511, 513]
SCALED_NZ = [1, 3]


def scaled_gram_written(D, ld):
    """[D][ld] bool, restated from the kernel: row r writes columns 0 .. r | 1 (the pairs c = 0, 2, ... with c <= r and c < D) -- for odd D
    that includes column D of row D - 1"""
    r, col = np.arange(D)[:, None], np.arange(ld)[None, :]
    return col <= (r | 1)


def scaled_gram_case(D, nz):
    """G0 [D + 2][ldg] NaN outside what is read (= the written set of a slot), inv_eta [nz + 2] NaN past nz, J [nz + 1][D + 2][ldj] NaN on entry;
    ldg and ldj even, >= D + 1 and different"""
    rng = np.random.default_rng(10 * D + nz)
    ldg, ldj = _round_up(D + 1, 2) + 2, _round_up(D + 1, 2)
    c = dict(D=D, nz=nz, ldg=ldg, ldj=ldj, rows=D + 2, cols=D + 1)
    read = scaled_gram_written(D, ldg)
    G0 = np.full((D + 2, ldg), np.nan)
    G0[:D][read] = rng.standard_normal(int(read.sum()))
    inv_eta = guarded_vec(rng.uniform(0.2, 3.0, nz), nz + 2)
    written = scaled_gram_written(D, D + 1)
    ref = np.where(written[None], G0[None, :D, :D + 1] * inv_eta[:nz, None, None], 0.0)
    c.update(G0=G0, inv_eta=inv_eta, written=np.broadcast_to(written, (nz, D, D + 1)).copy(), ref=ref)
    return c
