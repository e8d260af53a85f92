"""Cases, inputs and references of tests/test_gpu_contraction.py, built with CPU torch alone (tests/test_contraction_cases_host.py checks them
without a GPU).  The fp64 contraction template of pgl_gemm.hip, C = beta C + alpha A' diag(w) B, variant by variant.

The dispatch of pgl_launch_gemm is RESTATED here (gram_kernel, tile_variant, skinny_split) -- the tests choose their shapes from it:
    Gram      tiles = ntm (ntm + 1) / 2 with ntm = ceil(D / 128), items = tiles * ceil(nz / 2):
              items < 2 CUs -> gram_fine (4 waves, one neuron per item, tiles * nz items on 2 CUs workgroups), else the 8-wave pipeline
    plain     N <= 128 -> <2,2,1>;  else M <= 64 -> <1,4,1>;  else <2,4,1>;   every triangular product -> <2,2,1>
    CINIT     beta == 1 and alpha == +-1
    skinny    kernel >= 1, tri == 1, M > 128, M % 128 in 1..16: the last M % 128 rows through the skinny kernel, the tiles on the rest

Two kinds of operands.
  "exact"  dyadic: A, B, X, C0 entries k/8 with |k| <= 32 (about a quarter zero), weights m/4 with 0 <= m <= 16, alpha and beta from
           {1, -1, 2, -0.5, 0}.  Every product and partial sum is then an integer multiple of 2^-9 far below 2^52 for K <= 96, so every
           summation order gives the same fp64 bits: the reference is a CPU fp64 matmul and the comparison torch.equal (scaled_int_check
           proves the premise in int64).
  "real"   randn operands, weights rand / 4; element-wise bound (K + 4) 2^-53 (|beta| |C0| + |alpha| |A|' diag|w| |B|): the any-order bound of a
           length-K fp64 dot product (K u / (1 - K u) on the sum of magnitudes) plus the roundings of the scaling by alpha, the scaling by beta,
           the omega multiply and the final addition -- derived, not measured.
Poison: whatever the kernel must not write, and whatever it must not read into a stored value, is NaN; untouched regions are compared as int64
bit patterns (check_output)."""
import torch

F64 = torch.float64
NAN = float("nan")
U = 2.0 ** -53
KS = [16, 32, 48, 96]
ALPHA_BETA = [(1.0, 0.0), (-0.5, 0.0), (1.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, -0.5)]
CU_COUNTS = [64, 256, 304]
KINDS = ["exact", "real"]

# ------------------------------------------------------------------------------------------------------------ the dispatch, restated


def gram_tiles(D):
    ntm = -(-D // 128)
    return ntm * (ntm + 1) // 2


def gram_kernel(D, nz, cu):
    return "gram_fine" if gram_tiles(D) * ((nz + 1) // 2) < 2 * cu else "gram_wave8"


def gram_fine_items_per_workgroup(D, nz, cu):
    """(least, most) items a workgroup of the fine kernel can be handed: tiles * nz items over min(items, 2 cu) workgroups"""
    items = gram_tiles(D) * nz
    groups = min(items, 2 * cu)
    return items // groups, -(-items // groups)


def nz_wave8(D, cu):
    """the smallest odd nz whose launch runs the 8-wave pipeline"""
    nz = 1
    while gram_tiles(D) * ((nz + 1) // 2) < 2 * cu:
        nz += 2
    return nz


def nz_fine_second_item(cu):
    """an even nz with 3 nz / 2 < 2 cu < 3 nz (D = 130: three tiles): the fine kernel, and more items than its 2 cu workgroups"""
    return (150 * cu // 128) & ~1


def tile_variant(M, N, tri, alpha, beta):
    if tri:
        base = "tri<2,2,1>"
    elif N <= 128:
        base = "plain<2,2,1>"
    else:
        base = "plain<1,4,1>" if M <= 64 else "plain<2,4,1>"
    return base + (" cinit" if beta == 1.0 and alpha in (1.0, -1.0) else "")


def skinny_split(M, tri, kernel):
    return kernel >= 1 and tri == 1 and M > 128 and 1 <= M % 128 <= 16


VARIANTS = ["gram_fine", "gram_wave8", "skinny+tiles"] + [v + c for v in ("plain<2,2,1>", "plain<1,4,1>", "plain<2,4,1>", "tri<2,2,1>")
                                                           for c in ("", " cinit")]

# ------------------------------------------------------------------------------------------------------------------------- inputs


def _values(kind, g, shape):
    if kind == "real":
        return torch.randn(shape, dtype=F64, generator=g)
    k = torch.randint(-32, 33, shape, generator=g)
    return (k * (torch.rand(shape, generator=g) >= 0.25)).to(F64) / 8


def _weights(kind, g, shape):
    if kind == "real":
        return torch.rand(shape, dtype=F64, generator=g) * 0.25
    return torch.randint(0, 17, shape, generator=g).to(F64) / 4


def tile_mask(M, N, tri):
    """the elements of an M x N result whose 128 x 128 tile the product writes"""
    r, c = torch.arange(M)[:, None] // 128, torch.arange(N)[None, :] // 128
    if tri == 1:
        return r >= c
    if tri == 2:
        return c >= r
    return torch.ones(M, N, dtype=torch.bool)


def gram_case(kind, D, nz, Tp, seed=0):
    """X [Tp + 16][ldx] with NaN from column x_cols & ~1 on (x_cols is odd: one past the even count the kernel may read) and from row Tp on,
    W [Tp + 16][ldw] with NaN from column nz on and from row Tp on, J0 [nz][D][D] the start of an accumulating call; ref0 = X' diag(w_z) X on
    [nz][D][D], absP the same of magnitudes (real), written [nz][D][D] the lower tiles.  J has nz + 1 slots of ldj x ldj."""
    g = torch.Generator().manual_seed(1000 * D + 10 * Tp + nz + seed)
    De = D + (D & 1)
    c = dict(kind=kind, D=D, nz=nz, Tp=Tp, x_cols=De + 1, ldx=De + 4, ldw=nz + 3, ldj=D + 14)
    X, W = _values(kind, g, (Tp + 16, c["ldx"])), _weights(kind, g, (Tp + 16, c["ldw"]))
    X[:, De:] = NAN
    W[:, nz:] = NAN
    X[Tp:] = NAN                                   # one K tile of rows past Tp: a pipeline that consumes a tile too many stores NaN
    W[Tp:] = NAN
    Xd, Wd = X[:Tp, :D], W[:Tp, :nz]
    c.update(X=X, W=W, J0=_values(kind, g, (nz, D, D)), written=tile_mask(D, D, 1)[None].expand(nz, D, D))
    c["ref0"] = torch.matmul(Xd.T[None] * Wd.T[:, None, :], Xd)
    c["absP"] = torch.matmul(Xd.T[None].abs() * Wd.T[:, None, :], Xd.abs()) if kind == "real" else None
    return c


def gram_ref(c, accumulate):
    """(ref, bound or None) of pgl_weighted_gram on the case, from J0 where it accumulates"""
    ref = c["ref0"] + c["J0"] if accumulate else c["ref0"]
    if c["kind"] != "real":
        return ref, None
    return ref, (c["Tp"] + 4) * U * (c["absP"] + (c["J0"].abs() if accumulate else 0.0))


def contraction_case(kind, M, N, K, nb, alpha, beta, tri=0, batch_k=None, shared=False, full_cols=False, seed=0):
    """A [nb or 1][K][lda], B [nb or 1][K][ldb] (one shared pair: strides 0), values C0 [nb][M][N] of the written elements where beta != 0.
    a_cols, b_cols: odd, one past the even counts Me, Ne the kernel may read; columns from Me, Ne on are NaN, and so are the rows of a batch
    past its own K.  full_cols (pgl_activation): every column up to the leading dimension is readable and finite.  C has nb + 1 slots of
    rows x ldc.  ref, bound (real), written: [nb][M][N]; a batch with batch_k = 0 is not written at all."""
    g = torch.Generator().manual_seed(100000 * tri + 1000 * M + 7 * N + K + seed)
    Me, Ne = M + (M & 1), N + (N & 1)
    c = dict(kind=kind, M=M, N=N, K=K, nb=nb, alpha=alpha, beta=beta, tri=tri, batch_k=batch_k, shared=shared, lda=Me + 6, ldb=Ne + 4,
             ldc=N + 5, rows=M + 3, a_cols=Me + 1, b_cols=Ne + 1)
    na = 1 if shared else nb
    A, B = _values(kind, g, (na, K, c["lda"])), _values(kind, g, (na, K, c["ldb"]))
    if full_cols:
        c.update(a_cols=c["lda"], b_cols=c["ldb"])
    else:
        A[:, :, Me:] = NAN
        B[:, :, Ne:] = NAN
    if batch_k is not None and not shared:
        for b, kb in enumerate(batch_k):
            A[b, kb:] = NAN
            B[b, kb:] = NAN
    C0 = _values(kind, g, (nb, M, N))
    ref, bound = torch.empty(nb, M, N, dtype=F64), torch.zeros(nb, M, N, dtype=F64)
    written = tile_mask(M, N, tri)[None].repeat(nb, 1, 1)
    for b in range(nb):
        kb, s = (K if batch_k is None else batch_k[b]), (0 if shared else b)
        if kb == 0:
            written[b] = False
            ref[b] = C0[b]
            continue
        Ab, Bb = A[s, :kb, :M], B[s, :kb, :N]
        ref[b] = alpha * (Ab.T @ Bb) + (beta * C0[b] if beta != 0.0 else 0.0)
        bound[b] = (kb + 4) * U * (abs(alpha) * (Ab.abs().T @ Bb.abs()) + abs(beta) * C0[b].abs())
    c.update(A=A, B=B, C0=C0, ref=ref, bound=bound if kind == "real" else None, written=written)
    return c


# ------------------------------------------------------------------------------------------------------------------- the assertions


def poisoned_buffer(values, keep, slots, rows, ld):
    """[slots][rows][ld] of NaN with values [n][M][N] where keep: what the kernel is handed as C or J (on the device of `values`)"""
    n, M, N = values.shape
    buf = torch.full((slots, rows, ld), NAN, dtype=F64, device=values.device)
    buf[:n, :M, :N] = torch.where(keep, values, torch.full_like(values, NAN))
    return buf


def check_output(got, before, ref, bound, written, what=""):
    """got, before [slots][rows][ld] (after and before the call); ref, bound, written [n][M][N].  Written elements: torch.equal with ref (bound
    None), else |got - ref| <= bound and finite.  Every other element of the buffer: the same BITS as before."""
    n, M, N = ref.shape
    sub = got[:n, :M, :N]
    if bound is None:
        assert torch.equal(sub[written], ref[written]), "%s: %d written elements differ from the exact reference" % (
            what, int((sub[written] != ref[written]).sum()))
    else:
        err = (sub[written] - ref[written]).abs()
        bad = ~(err <= bound[written])          # (a NaN fails)
        assert not bool(bad.any()), "%s: %d elements beyond the bound, worst |err| / bound = %.3g" % (
            what, int(bad.sum()), float((err / bound[written])[bad].nan_to_num(nan=float("inf")).max()))
    expect = before.clone()
    expect[:n, :M, :N] = torch.where(written, sub, before[:n, :M, :N])
    same = expect.view(torch.int64) == got.view(torch.int64)
    assert bool(same.all()), "%s: %d elements outside the written set changed" % (what, int((~same).sum()))


def scaled_int_check(A, B, w, C0, alpha, beta, ref):
    """The premise of the exact cases, for one A [K][M], B [K][N], w [K] or None, C0 [M][N]: with A = A8 / 8, B = B8 / 8, w = w4 / 4, C0 = C8 / 8,
    alpha = a2 / 2, beta = b2 / 2 all integers, ref * den == a2 sum_k A8 w4 B8 + b2 C8 (den / 16) in int64, den = 128 (512 with weights).
    Returns the largest magnitude any partial sum can reach in those units, a2 |A8|' |w4| |B8| + |b2| |C8| den / 16: below 2^52 every partial
    sum of every summation order is an exactly representable fp64 number."""
    def ints(t, s):
        i = (t * s).round().to(torch.int64)
        assert torch.equal(i.to(F64) / s, t), "an operand is not a multiple of 1 / %d" % s
        return i
    A8, B8, C8 = ints(A, 8), ints(B, 8), ints(C0, 8)
    w4 = ints(w, 4) if w is not None else torch.ones(A.shape[0], dtype=torch.int64)
    a2, b2 = ints(torch.tensor(alpha, dtype=F64), 2), ints(torch.tensor(beta, dtype=F64), 2)
    den = 512 if w is not None else 128
    exact = a2 * ((A8 * w4[:, None]).T @ B8) + b2 * C8 * (den // 16)
    assert torch.equal(ref * den, exact.to(F64)), "the fp64 reference is not the integer result"
    return int((a2.abs() * ((A8.abs() * w4[:, None]).T @ B8.abs()) + b2.abs() * C8.abs() * (den // 16)).max())


# ------------------------------------------------------------------------------------------------------------------- the case lists

GRAM_WAVE8 = [(D, Tp) for D in (130, 256) for Tp in (16, 32, 48, 64, 80)]                  # 1 .. 5 K tiles around the three stages
GRAM_FINE = [(D, nz) for D in (1, 2, 17, 127, 128, 129, 130, 384) for nz in (1, 2, 3)]
GRAM_FINE_TP = [16, 32, 48, 64]                                                            # 2, 4, 6, 8 eight-row stages around the four
GRAM_FINE_MULTI_TP = [16, 48]

PLAIN_SHAPES = {"plain<2,2,1>": [(128, 128), (129, 128), (200, 1), (130, 127)],
                "plain<1,4,1>": [(1, 129), (17, 300), (64, 256), (64, 257)],
                "plain<2,4,1>": [(65, 129), (130, 300)]}
TRI_M = [1, 127, 128, 129, 200]
SKINNY_M = [129, 144, 145, 258]
NBATCH = 3


def _rotate(family, shapes, tri=0, kernel=0, pairs=ALPHA_BETA, shared=False):
    """every shape with every (alpha, beta); K walks KS and batch_k switches every four cases, so every (family, K) and (family, alpha / beta) occurs"""
    out = []
    for M, N in shapes:
        for alpha, beta in pairs:
            i = len(out)
            K = KS[i % 4]
            out.append(dict(family=family, M=M, N=N, K=K, alpha=alpha, beta=beta, tri=tri, kernel=kernel, shared=shared,
                            batch_k=[K, 16, 0] if (i // 4) % 2 else None,
                            variant="skinny+tiles" if skinny_split(M, tri, kernel) else tile_variant(M, N, tri, alpha, beta)))
    return out


def batched_cases():
    cases = []
    for family, shapes in PLAIN_SHAPES.items():
        cases += _rotate(family, shapes)
    for tri in (1, 2):
        cases += _rotate("tri%d" % tri, [(M, M) for M in TRI_M], tri=tri)
    cases += _rotate("shared", [(130, 300)], shared=True)
    for c in cases:
        c["id"] = "%s-%dx%d-K%d-a%g-b%g%s" % (c["family"], c["M"], c["N"], c["K"], c["alpha"], c["beta"], "-bk" if c["batch_k"] else "")
    return cases


def skinny_cases():
    cases = _rotate("skinny", [(M, M) for M in SKINNY_M] * 2, tri=1, kernel=1, pairs=[(-1.0, 1.0)])     # (twice: each M with and without batch_k)
    for c in cases:
        c["id"] = "skinny-%d-K%d%s" % (c["M"], c["K"], "-bk" if c["batch_k"] else "")
    return cases


ACTIVATION = [(T, nloc, Dk) for T in (1, 77, 128, 200) for nloc in (1, 3, 128, 130) for Dk in (16, 48)]
BORDER = [(M, N, beta) for M in (2, 64, 66) for N in (17, 129) for beta in (0.0, 1.0)]


def border_K(M, N, beta):
    return KS[(BORDER.index((M, N, beta))) % 4]
