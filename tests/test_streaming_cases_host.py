"""The cases, references and emulations of tests/_streaming_cases.py against brute force on the CPU (no GPU): what tests/test_gpu_streaming.py
holds the kernels to is itself held to loops written out cell by cell, to math.fsum and to int64 arithmetic.  Also here: the mutations of a
reference that stand for a broken kernel (a row late in the convolution, another wave order, the upper triangle in the assembly) do change it."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import _streaming_cases as S


# ------------------------------------------------------------------------------------------------------------------ geometry
def test_geometry_restated():
    assert S.PGLL_ROWS == 64 and [S.psi_row_blocks(T) for T in (1, 64, 65, 257)] == [1, 1, 2, 5]
    assert [S.psi_narrow(n, 0) for n in (1, 63, 64, 65)] == [True, True, False, False] and not S.psi_narrow(5, 2)
    assert S.conv_blocks(37, 7) == 2 and S.conv_blocks(64, 4) == 1 and 256 % 7 != 0
    assert S.assembly_chunks(51, 5) == 1 and S.assembly_chunks(64, 4) == 2          # column D = 255: last thread of chunk 0; D = 256: first of chunk 1
    assert S.transpose_tiles(33, 70) == (2, 3) and S.transpose_tiles(32, 32) == (1, 1)
    assert S.conv_lds_bytes(*S.DESIGN_LDS_SHAPE[:1:-1]) == 65792 > S.LDS_DEFAULT and S.conv_lds_bytes(*S.DESIGN_LDS_REFUSED[:1:-1]) > S.LDS_MAX
    assert S.pg_stream(3, 1005) == 3 * 2 ** 32 + 1005
    # every T edge with a narrow and a wide walk, every nloc edge at T = 130
    for T in S.PSI_T:
        assert (T, 5) in S.PSI_SHAPES and (T, 65) in S.PSI_SHAPES
    assert all((130, n) in S.PSI_SHAPES for n in S.PSI_NLOC) and len(S.PSI_SHAPES) == 16
    assert all(p in S.PSI_SHAPES for p in S.PSI_PRODUCTION)


def test_guards():
    g = S.guarded(np.ones((2, 3)), 4, 5)
    assert np.isnan(g[2:]).all() and np.isnan(g[:, 3:]).all() and (g[:2, :3] == 1).all()
    S.same_bits(g, g.copy())
    h = g.copy()
    h[0, 0] = -0.0
    g[0, 0] = 0.0
    with pytest.raises(AssertionError):
        S.same_bits(g, h)


# ------------------------------------------------------------------------------------------------------------------ A
def _conv_brute(Sm, basis, clip):
    T, N = Sm.shape
    R, B = basis.shape
    X = np.zeros((T, N * B + 1))
    for t in range(T):
        for n in range(N):
            for b in range(B):
                v = math.fsum(basis[l, b] * Sm[t - 1 - l, n] for l in range(min(R, t)))
                X[t, n * B + b] = max(v, 0.0) if clip else v
        X[t, N * B] = 1.0
    return X


@pytest.mark.parametrize("T,N,B,R", S.DESIGN_SHAPES[:3] + [(65, 4, 1, 1), (12, 2, 3, 40)])
@pytest.mark.parametrize("kind", S.KINDS)
def test_design_reference_against_loops(kind, T, N, B, R):
    c = S.design_case(kind, T, N, B, R)
    assert c["lds"] > N and c["ldx"] > N * B + 1 and c["ldxt"] > T and ((c["basis"] < 0).any() or R * B == 1)
    assert np.isnan(c["S_buf"][:, N:]).all() and np.isnan(c["S_buf"][T:]).all()
    for clip in (0, 1):
        ref, mag = S.design_ref(c["S"], c["basis"], clip)
        brute = _conv_brute(c["S"], c["basis"], clip)
        if kind == "exact":
            assert np.array_equal(ref.astype(np.float64), brute)           # products exact, fsum exact
        else:
            assert (np.abs(ref - brute) <= 2 * S.U * mag + 1e-300).all()
        assert (ref[0, :-1] == 0).all() and (ref[:, -1] == 1).all()
    # the mutation "t - 1 -> t" (an acausal kernel) is another matrix
    late = np.vstack([c["S"][1:], np.zeros((1, N))])
    if T > 1 and np.abs(c["S"]).sum() > 0:
        assert not np.array_equal(S.design_ref(late, c["basis"], 0)[0], S.design_ref(c["S"], c["basis"], 0)[0])


@pytest.mark.parametrize("T,N,B,R", S.DESIGN_SHAPES + [S.DESIGN_LDS_SHAPE])
def test_exact_design_operands_are_exact(T, N, B, R):
    """dyadic operands: the sum is the same fp64 number in every order of addition (here: forward, backward and a random order, in fp64)"""
    c = S.design_case("exact", T, N, B, R)
    assert S.conv_exact_premise(c["S"], c["basis"]) * 1024 < 2 ** 53
    ref = S.design_ref(c["S"], c["basis"], 0)[0].astype(np.float64)
    rng = np.random.default_rng(0)
    for t, n, b in {(T - 1, N - 1, B - 1), (T // 2, 0, 0), (min(T - 1, R), N // 2, B // 2)}:
        terms = [c["basis"][l, b] * c["S"][t - 1 - l, n] for l in range(min(R, t))]
        for order in (terms, terms[::-1], list(rng.permutation(terms))):
            acc = 0.0
            for v in order:
                acc += v
            assert acc == ref[t, n * B + b]


@pytest.mark.parametrize("T,N,B,R", S.DESIGN_SHAPES)
def test_block_with_history_is_the_rows_of_the_whole(T, N, B, R):
    c = S.design_case("real", T, N, B, R)
    whole = S.design_ref(c["S"], c["basis"], 0)[0]
    blocks = S.history_blocks(T, R)
    assert blocks and all(0 <= r0 < r1 <= T for r0, r1 in blocks)
    for r0, r1 in blocks:
        h = min(R, r0)
        part = S.design_ref(c["S"][r0 - h:r1], c["basis"], 0)[0]
        assert part.shape[0] == r1 - r0 + h and np.array_equal(part[h:], whole[r0:r1])


# ------------------------------------------------------------------------------------------------------------------ B
def test_transpose_cases():
    assert len(S.TRANSPOSE_SHAPES) == 20
    c = S.transpose_case(33, 70)
    assert c["ld_src"] > 70 and c["ld_dst"] > 33 and np.isnan(c["src"][33:]).all() and np.isnan(c["src"][:, 70:]).all()
    assert np.signbit(c["values"][c["values"] == 0]).any() and c["values"][0, 0] == 5e-324


# ------------------------------------------------------------------------------------------------------------------ C
def test_reduction_emulation_against_a_plain_sum():
    rng = np.random.default_rng(1)
    for T in S.PSI_T:
        terms = rng.standard_normal((T, 7)) * 10.0 ** rng.integers(-3, 4, (T, 7))
        out, part = S.emulate_reduction(terms)
        assert part.shape == (S.psi_row_blocks(T), 7)
        exact = np.array([math.fsum(terms[:, n]) for n in range(7)])
        assert (np.abs(out - exact) <= (T // 64 + 20) * S.U * np.abs(terms).sum(axis=0)).all()
        for blk in range(part.shape[0]):          # a block's partial is the sum of its rows
            rows = terms[blk * 64:(blk + 1) * 64]
            assert (np.abs(part[blk] - [math.fsum(rows[:, n]) for n in range(7)]) <= 20 * S.U * np.abs(rows).sum(axis=0)).all()
        out1, _ = S.emulate_reduction(terms, out0=np.arange(7.0))
        assert np.array_equal(out1, np.arange(7.0) + out)
    # dyadic terms: exact whatever the order
    k = rng.integers(-1000, 1000, (257, 5)) / 64.0
    assert np.array_equal(S.emulate_reduction(k)[0], k.sum(axis=0))


def test_reduction_emulation_written_out_for_one_block():
    """T = 9: wave 0 rows 0, 4, 8; wave 1 rows 1, 5; wave 2 rows 2, 6; wave 3 rows 3, 7"""
    x = np.random.default_rng(2).standard_normal((9, 1))[:, 0]
    r0, r1, r2, r3 = ((0.0 + x[0]) + x[4]) + x[8], (0.0 + x[1]) + x[5], (0.0 + x[2]) + x[6], (0.0 + x[3]) + x[7]
    out, part = S.emulate_reduction(x[:, None])
    assert part[0, 0] == ((r0 + r1) + r2) + r3 and out[0] == 0.0 + part[0, 0]


def test_reduction_emulation_notices_another_order():
    """the order is what the device tests pin: swapping two waves, or adding the rows in sequence, changes bits of some column"""
    terms = np.random.default_rng(3).standard_normal((130, 64))
    out, _ = S.emulate_reduction(terms)
    assert (S.emulate_reduction(terms, wave_order=(0, 2, 1, 3))[0] != out).any()
    assert (S.emulate_reduction(terms, wave_order=(3, 2, 1, 0))[0] != out).any()
    seq = np.zeros(64)
    for t in range(130):
        seq = seq + terms[t]
    assert (seq != out).any()


@pytest.mark.parametrize("variant", list(S.PSI_VARIANTS))
@pytest.mark.parametrize("T,nloc", [(65, 5), (130, 65)])
def test_loglik_reference_and_cap(variant, T, nloc):
    """the reference's log c without lgamma against the formula with lgamma, in NumPy fp64: under the cap the device is held to"""
    c = S.psi_case(T, nloc, variant)
    psi_out = c["psi"] + c["bias"]
    assert np.abs(psi_out).max() <= 30 and c["layout"] == ("production" if (T, nloc) in S.PSI_PRODUCTION else "unrelated")
    l, cap = S.ll_reference(c, psi_out)
    ratio = np.abs(S.ll_formula_fp64(c, psi_out) - l) / np.where(cap > 0, cap, 1) * 16
    assert np.isfinite(np.asarray(l, dtype=np.float64)).all() and (ratio <= 16).all(), "worst %.3g units of the 16" % ratio.max()
    # the cap separates a wrong operand from rounding: the neighbouring cell's y, or b off by one, is beyond 2^30 units nearly everywhere
    if c["obs"] in (1, 3) and nloc > 1:
        other = dict(c, Y=np.roll(c["Y"], 1, axis=1), a=np.roll(c["a"], 1, axis=1))
        if c["obs"] == 3:
            other["Y"] = np.minimum(other["Y"], c["p"])
            other["a"] = other["Y"]
        else:
            other["b"] = other["Y"] + c["p"]
        wrong = np.abs(S.ll_formula_fp64(other, psi_out) - l)
        differs = other["Y"] != c["Y"]
        assert differs.any() and (wrong[differs] > 2.0 ** 30 / 16 * cap[differs]).mean() > 0.99
    # the guards: nothing finite in a padding column
    assert np.isnan(c["Psi_buf"][:, nloc:]).all() and np.isnan(c["Y_buf"][T:]).all() and np.isnan(c["bias_buf"][nloc:]).all()
    if c["hooks"] is not None:
        h = c["hooks"].reshape(T, 3, c["ldh"])
        assert np.isnan(h[:, :, nloc:]).all() and np.array_equal(h[:, 1, :nloc], c["b"]) and c["ldh"] > nloc
    if c["layout"] == "production":
        assert c["ldo"] == c["ldk"] == 2 * c["ldn"] and c["ok_rows"] == -(-T // 16) * 16 + 1 and c["ldn"] >= nloc


def test_loglik_reference_against_exact_rational_arithmetic():
    """log c of a few cells from Fractions: the binomial coefficient, and prod_{k < y} (xi + k) / (k + 1) for the negative binomial"""
    for variant in ("negbin_param", "binomial_param"):
        c = S.psi_case(65, 5, variant)
        zero = np.zeros_like(c["psi"])
        l, _ = S.ll_reference(c, zero)                 # psi = 0: l = log c - b log 2
        logc = l + c["b"].astype(S.LD) * np.log(S.LD(2))
        for t in range(0, 65, 7):
            for n in range(5):
                y, p = int(c["Y"][t, n]), c["p"][n]
                if variant == "binomial_param":
                    exact = Fraction(math.comb(int(p), y))
                else:
                    exact = Fraction(1)
                    for k in range(y):
                        exact *= (Fraction(float(p)) + k) / (k + 1)
                assert abs(float(logc[t, n]) - math.log(exact)) <= 1e-13 * (1 + abs(math.log(exact)))


def test_hooks_of_bernoulli():
    c = S.psi_case(65, 5, "bernoulli")
    h = S.hooks_of_bernoulli(c).reshape(65, 3, c["ldh"])
    assert np.array_equal(h[:, 0, :5], c["Y"]) and (h[:, 1, :5] == 1).all() and (h[:, 2, :5] == 0).all() and np.isnan(h[:, :, 5:]).all()


@pytest.mark.parametrize("T,nloc", S.GAUSS_SHAPES)
def test_gaussian_residuals_are_exact_and_their_sums_are_not(T, nloc):
    c = S.gauss_case(T, nloc)
    sq = S.gauss_exact_premise(c)
    out, _ = S.emulate_reduction(sq)
    exact = np.array([math.fsum(sq[:, n]) for n in range(nloc)])
    assert (np.abs(out - exact) <= (T // 64 + 20) * S.U * exact).all()
    if T >= 63:
        assert (out != exact).any() or (S.emulate_reduction(sq, wave_order=(3, 2, 1, 0))[0] != out).any()      # the sums do round: the order shows


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("N,B", [(3, 2), (1, 1), (8, 32), (51, 5)])
def test_assembly_reference_against_loops(N, B):
    c = S.assemble_case(N, B, 3)
    D = N * B
    tri = c["tri"]
    assert tri.sum() == N * B * (B + 1) // 2 and not tri[D:].any() and not tri[:, D:].any()
    assert all(tri[r, col] == (col // B == r // B and col <= r) for r in range(0, D, max(1, D // 7)) for col in range(D))
    assert np.isnan(c["J"][3]).all() and np.isfinite(c["J"][:3][:, tri]).all() and np.isnan(c["J"][:3][:, ~tri]).all()
    assert np.isnan(c["bo"][:, D + 1:]).all() and np.isnan(c["bk"][3]).all() and c["ldj"] > D + 2 and c["rows"] > D + 2
    with np.errstate(invalid="ignore"):
        assert (S.bits(c["J"][3]) == S.SNAN_BITS).all() and (S.bits(c["J"].copy() + 1.0)[3] != S.SNAN_BITS).all()  # copies keep the bits, an addition does not
    ref = S.assemble_ref(c, c["Jw"], c["hw"])
    for n in range(3):
        for r in range(0, D, max(1, D // 5)):
            m = r // B
            for col in range(m * B, r + 1):
                assert ref[n, r, col] == c["J"][n, r, col] + c["Jw"][n, m, r % B, col - m * B]
            assert ref[n, D + 1, r] == c["bk"][n, r] + c["hw"][n, m, r % B] and ref[n, D, r] == c["bo"][n, r]
        assert ref[n, D, D] == c["bo"][n, D] + c["Jb"][n] and ref[n, D + 1, D] == c["bk"][n, D] + c["hb"][n] and ref[n, D + 1, D + 1] == 0
    changed = S.bits(ref) != S.bits(c["J"])
    expect = np.zeros_like(changed)
    expect[:3] = tri
    expect[:3, D, :D + 1] = True
    expect[:3, D + 1, :D + 2] = True
    assert not (changed & ~expect).any()
    # the tables expand to a dense prior of the dense layout; a kernel that also adds the upper triangle gives another J
    assert c["Jw_expanded"].shape == c["Jw"].shape and c["hw_expanded"].shape == c["hw"].shape
    assert all(np.array_equal(c["Jw_expanded"][n, m], c["Jw_table"][c["label"][n, m]]) for n in range(3) for m in range(N))
    if B > 1:
        assert len(set(c["label"].ravel())) > 1 or N == 1


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("D", S.SCALED_D)
def test_scaled_gram_written_set_against_the_thread_loop(D):
    """the kernel's own loop over (row, thread), restated: c = 2 * thread, skip c > r or c >= D, write c and c + 1"""
    c = S.scaled_gram_case(D, 3)
    mask = np.zeros((D, c["ldj"]), dtype=bool)
    for r in range(D):
        for col in range(0, 2 * ((D // 2 + 255) // 256 + 1) * 256, 2):
            if col > r or col >= D:
                continue
            mask[r, col:col + 2] = True
    assert np.array_equal(mask, S.scaled_gram_written(D, c["ldj"])) and c["ldj"] >= D + 1 and c["ldg"] >= D + 1 and c["ldj"] % 2 == c["ldg"] % 2 == 0
    assert mask[D - 1, D] == bool(D & 1) and c["ldg"] != c["ldj"]
    assert np.array_equal(np.isfinite(c["G0"][:D]), S.scaled_gram_written(D, c["ldg"])) and np.isnan(c["G0"][D:]).all() and np.isnan(c["inv_eta"][3:]).all()
    w = c["written"]
    assert np.isfinite(c["ref"][w]).all() and c["ref"][1, D - 1, 0] == c["G0"][D - 1, 0] * c["inv_eta"][1]
