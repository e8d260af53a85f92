"""The fp64 contraction kernels of pgl_gemm.hip variant by variant, through the C ABI alone (pgl_weighted_gram, pgl_contract_tn_batched,
pgl_contract_tn, pgl_activation): each variant of pgl_launch_gemm's dispatch at shapes of a few tiles, against a CPU fp64 reference.
tests/_contraction_cases.py holds the cases, the references and the assertions (and restates the dispatch the shapes are chosen from);
tests/test_contraction_cases_host.py checks those without a GPU.  Every case runs twice: on dyadic operands, where every summation order
gives the same bits and the comparison is torch.equal, and on real ones, element-wise within (K + 4) 2^-53 (|beta| |C0| + |alpha| |A|' |w| |B|).
Whatever must not be written -- rows and columns past M, N, D up to the leading dimension, tiles on the other side of the diagonal, a
skipped batch, one whole slot after the last -- and whatever must not be read -- operand columns from a_cols / x_cols on, weight columns from
nz on, rows of a batch past its own K, one K tile of rows of X and W past Tp -- is NaN, and the untouched regions are compared as bit patterns.  The real operands also carry the
bit-for-bit comparisons between variants: the 8-wave Gram against the fine one, the skinny-row split against the tiles, the 64-row and the
128-column tile against the 128 x 256 one."""
import pytest

from tests import _contraction_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gram(c, X, W, J, nz, accumulate):
    import torch
    from pyglm_amd._lib import call, ptr
    call("pgl_weighted_gram", X=ptr(X), ldx=c["ldx"], x_cols=c["x_cols"], W=ptr(W), ldw=c["ldw"], Tp=c["Tp"], D=c["D"], nz=nz, J=ptr(J),
         ldj=c["ldj"], strideJ=c["ldj"] * c["ldj"], accumulate=accumulate, hip_stream=None)
    torch.cuda.synchronize()


def _check_gram(kind, D, nz, Tp, same_bits_with_fine=False):
    """both values of `accumulate` on one case: J of nz + 1 slots of ldj x ldj, NaN but for the lower tiles of an accumulating call"""
    import torch
    c = C.gram_case(kind, D, nz, Tp)
    X, W, written, J0 = c["X"].to(DEV), c["W"].to(DEV), c["written"].to(DEV), c["J0"].to(DEV)
    for accumulate in (0, 1):
        ref, bound = C.gram_ref(c, accumulate)
        before = C.poisoned_buffer(J0, written if accumulate else torch.zeros_like(written), nz + 1, c["ldj"], c["ldj"])
        J = before.clone()
        _gram(c, X, W, J, nz, accumulate)
        C.check_output(J, before, ref.to(DEV), None if bound is None else bound.to(DEV), written,
                       "%s Gram D = %d nz = %d Tp = %d accumulate = %d" % (kind, D, nz, Tp, accumulate))
        if same_bits_with_fine and accumulate == 0:
            # the first four neurons again in a launch of their own, which runs the fine kernel: a shard against the whole model
            J4 = before[:5].clone()
            _gram(c, X, W, J4, 4, 0)
            assert torch.equal(J4[:4, :D, :D][written[:4]], J[:4, :D, :D][written[:4]]), "the 8-wave and the fine Gram differ in bits"
            assert torch.equal(J4[4].view(torch.int64), before[4].view(torch.int64))


# ---------------------------------------------------------------------------------------------------------------- A. weighted Gram
@pytest.mark.parametrize("D,Tp", C.GRAM_WAVE8)
def test_gram_8wave_pipeline(D, Tp):
    """odd nz, just enough for the 8-wave pipeline on this device: 1 .. 5 K tiles around its three stages, several items per workgroup, the
    second wave group of the last pair storing nothing (the buffer ends one poisoned slot after slot nz - 1); on the real operands its first
    four neurons equal the fine kernel's bit for bit"""
    cu = _cus()
    nz = C.nz_wave8(D, cu)
    assert C.gram_kernel(D, nz, cu) == "gram_wave8" and C.gram_kernel(D, 4, cu) == "gram_fine" and nz % 2 == 1
    _check_gram("exact", D, nz, Tp)
    _check_gram("real", D, nz, Tp, same_bits_with_fine=True)


@pytest.mark.parametrize("D,nz", C.GRAM_FINE)
def test_gram_fine_pipeline_one_item_per_workgroup(D, nz):
    cu = _cus()
    assert C.gram_kernel(D, nz, cu) == "gram_fine" and C.gram_fine_items_per_workgroup(D, nz, cu) == (1, 1)
    for Tp in C.GRAM_FINE_TP:
        for kind in C.KINDS:
            _check_gram(kind, D, nz, Tp)


@pytest.mark.parametrize("Tp", C.GRAM_FINE_MULTI_TP)
def test_gram_fine_pipeline_several_items_per_workgroup(Tp):
    """more items than workgroups: an item's last DMA requests are still in flight into a stage the next item's prologue refills"""
    cu = _cus()
    nz = C.nz_fine_second_item(cu)
    assert C.gram_kernel(130, nz, cu) == "gram_fine" and C.gram_fine_items_per_workgroup(130, nz, cu) == (1, 2)
    for kind in C.KINDS:
        _check_gram(kind, 130, nz, Tp)


# --------------------------------------------------------------------------------------------------------- B. batched contraction
def _batched(c, A, B, Cbuf, kernel=0, M=None, N=None):
    import torch
    from pyglm_amd._lib import call, ptr
    bk = None if c["batch_k"] is None else torch.tensor(c["batch_k"], dtype=torch.int32, device=DEV)
    call("pgl_contract_tn_batched", A=ptr(A), lda=c["lda"], strideA=0 if c["shared"] else c["K"] * c["lda"], a_cols=c["a_cols"], B=ptr(B),
         ldb=c["ldb"], strideB=0 if c["shared"] else c["K"] * c["ldb"], b_cols=c["b_cols"], C=ptr(Cbuf), ldc=c["ldc"], strideC=c["rows"] * c["ldc"],
         M=M or c["M"], N=N or c["N"], K=c["K"], nbatch=c["nb"], batch_k=ptr(bk), alpha=c["alpha"], beta=c["beta"], tri=c["tri"], kernel=kernel,
         hip_stream=None)
    torch.cuda.synchronize()


def _before(c):
    """C as the kernel gets it: NaN but for the elements it reads (the written set where beta != 0)"""
    import torch
    written = c["written"].to(DEV)
    return C.poisoned_buffer(c["C0"].to(DEV), written if c["beta"] != 0.0 else torch.zeros_like(written), c["nb"] + 1, c["rows"], c["ldc"]), written


def _check_batched(case, kind, kernel=0):
    c = C.contraction_case(kind, case["M"], case["N"], case["K"], C.NBATCH, case["alpha"], case["beta"], tri=case["tri"], batch_k=case["batch_k"],
                           shared=case["shared"])
    A, B = c["A"].to(DEV), c["B"].to(DEV)
    before, written = _before(c)
    got = before.clone()
    _batched(c, A, B, got, kernel)
    C.check_output(got, before, c["ref"].to(DEV), None if c["bound"] is None else c["bound"].to(DEV), written, "%s %s kernel %d" % (kind, case["id"], kernel))
    return c, A, B, before, got


@pytest.mark.parametrize("case", C.batched_cases(), ids=lambda c: c["id"])
def test_batched_contraction(case):
    """<2,2,1>, <1,4,1>, <2,4,1>, both triangles and shared operands, each plain, read-modify-write and CINIT (alpha = +-1, beta = 1)"""
    for kind in C.KINDS:
        _check_batched(case, kind)


@pytest.mark.parametrize("case", C.skinny_cases(), ids=lambda c: c["id"])
def test_skinny_row_split_equals_the_tiles(case):
    """kernel = 1 on a lower triangle with 1 .. 16 rows past a multiple of 128: those rows through the skinny kernel (M = 145 is just past the
    split and runs the tiles alone).  Exact on dyadic data, and the bits of kernel = 0 on real data."""
    import torch
    _check_batched(case, "exact", kernel=1)
    c, A, B, before, got = _check_batched(case, "real", kernel=1)
    tiles = before.clone()
    _batched(c, A, B, tiles, 0)
    assert torch.equal(got.view(torch.int64), tiles.view(torch.int64)), "the skinny-row split and the tiles differ in bits"


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (2.0, 1.0)])
def test_tile_shapes_give_the_same_bits(alpha, beta):
    """rows [0, 64) of a 130 x 300 product (<2,4,1>) against M = 64 (<1,4,1>) and its columns [0, 128) against N = 128 (<2,2,1>), same operands"""
    import torch
    c = C.contraction_case("real", 130, 300, 96, C.NBATCH, alpha, beta)
    assert [C.tile_variant(M, N, 0, 0.0, 0.0) for M, N in ((130, 300), (64, 300), (130, 128))] == ["plain<2,4,1>", "plain<1,4,1>", "plain<2,2,1>"]
    A, B = c["A"].to(DEV), c["B"].to(DEV)
    before, written = _before(c)
    whole, rows, cols = before.clone(), before.clone(), before.clone()
    _batched(c, A, B, whole)
    _batched(c, A, B, rows, M=64)
    _batched(c, A, B, cols, N=128)
    C.check_output(whole, before, c["ref"].to(DEV), c["bound"].to(DEV), written, "130 x 300")
    nb = c["nb"]
    assert torch.equal(rows[:nb, :64, :300], whole[:nb, :64, :300]), "the 64-row tile and the 128-row tile differ in bits"
    assert torch.equal(cols[:nb, :130, :128], whole[:nb, :130, :128]), "the 128-column tile and the 256-column tile differ in bits"
    # and the smaller products wrote nothing past their own rows / columns
    keep = torch.zeros_like(before, dtype=torch.bool)
    keep[:nb, :64, :300] = True
    assert torch.equal(rows.view(torch.int64)[~keep], before.view(torch.int64)[~keep])
    keep[:] = False
    keep[:nb, :130, :128] = True
    assert torch.equal(cols.view(torch.int64)[~keep], before.view(torch.int64)[~keep])


# ---------------------------------------------------------------------------------------------------------- C. single contractions
@pytest.mark.parametrize("T,nloc,Dk", C.ACTIVATION)
def test_activation(T, nloc, Dk):
    """Psi = Xt' Wt with ldxt > T and ldpsi > nloc; every column up to ldxt / ldw is readable here, Psi past T rows / nloc columns is not written"""
    import torch
    from pyglm_amd._lib import call, ptr
    for kind in C.KINDS:
        c = C.contraction_case(kind, T, nloc, Dk, 1, 1.0, 0.0, full_cols=True)
        assert c["lda"] > T and c["ldc"] > nloc
        A, B = c["A"].to(DEV), c["B"].to(DEV)
        before, written = _before(c)
        got = before.clone()
        call("pgl_activation", Xt=ptr(A), ldxt=c["lda"], Wt=ptr(B), ldw=c["ldb"], Psi=ptr(got), ldpsi=c["ldc"], T=T, Dk=Dk, nloc=nloc, hip_stream=None)
        torch.cuda.synchronize()
        C.check_output(got, before, c["ref"].to(DEV), None if c["bound"] is None else c["bound"].to(DEV), written, "%s activation" % kind)


@pytest.mark.parametrize("M,N,beta", C.BORDER)
def test_contract_tn_in_the_border_sum_shape(M, N, beta):
    import torch
    from pyglm_amd._lib import call, ptr
    for kind in C.KINDS:
        c = C.contraction_case(kind, M, N, C.border_K(M, N, beta), 1, 1.0, beta)
        A, B = c["A"].to(DEV), c["B"].to(DEV)
        before, written = _before(c)
        got = before.clone()
        call("pgl_contract_tn", A=ptr(A), lda=c["lda"], a_cols=c["a_cols"], B=ptr(B), ldb=c["ldb"], b_cols=c["b_cols"], C=ptr(got), ldc=c["ldc"], M=M,
             N=N, K=c["K"], alpha=1.0, beta=beta, hip_stream=None)
        torch.cuda.synchronize()
        C.check_output(got, before, c["ref"].to(DEV), None if c["bound"] is None else c["bound"].to(DEV), written, "%s border sums" % kind)


# ------------------------------------------------------------------------------------------------------ D. the column-count contract
@pytest.mark.parametrize("entry", ["pgl_weighted_gram", "pgl_contract_tn-a", "pgl_contract_tn-b", "pgl_contract_tn_batched-a", "pgl_contract_tn_batched-b"])
def test_too_few_readable_columns_are_refused_and_nothing_is_launched(entry):
    """x_cols / a_cols / b_cols rounded down to even is less than D / M / N (an odd count equal to the dimension): PglError, C keeps its NaN"""
    import torch
    from pyglm_amd._lib import PglError, call, ptr
    M = N = D = 65
    X = torch.ones(16, 72, dtype=torch.float64, device=DEV)
    W = torch.ones(16, 2, dtype=torch.float64, device=DEV)
    out = torch.full((2, 72, 72), C.NAN, dtype=torch.float64, device=DEV)
    a_cols, b_cols = (65, 66) if entry.endswith("-a") else (66, 65)
    with pytest.raises(PglError):
        if entry == "pgl_weighted_gram":
            call("pgl_weighted_gram", ptr(X), 72, 65, ptr(W), 2, 16, D, 1, ptr(out), 72, 72 * 72, 0, None)
        elif entry.startswith("pgl_contract_tn_batched"):
            call("pgl_contract_tn_batched", ptr(X), 72, 0, a_cols, ptr(X), 72, 0, b_cols, ptr(out), 72, 72 * 72, M, N, 16, 1, None, 1.0, 0.0, 0, 0, None)
        else:
            call("pgl_contract_tn", ptr(X), 72, a_cols, ptr(X), 72, b_cols, ptr(out), 72, M, N, 16, 1.0, 0.0, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the same calls with 66 readable columns go through
    if entry == "pgl_weighted_gram":
        call("pgl_weighted_gram", ptr(X), 72, 66, ptr(W), 2, 16, D, 1, ptr(out), 72, 72 * 72, 0, None)
    elif entry.startswith("pgl_contract_tn_batched"):
        call("pgl_contract_tn_batched", ptr(X), 72, 0, 66, ptr(X), 72, 0, 67, ptr(out), 72, 72 * 72, M, N, 16, 1, None, 1.0, 0.0, 0, 0, None)
    else:
        call("pgl_contract_tn", ptr(X), 72, 67, ptr(X), 72, 66, ptr(out), 72, M, N, 16, 1.0, 0.0, None)
    torch.cuda.synchronize()
    assert bool((out[0, :65, :65] == 16.0).all()) and bool(torch.isnan(out[1]).all()) and bool(torch.isnan(out[0, 65:]).all())
