"""The lagged products on the GPU (pgl_lagged_products, pyglm_amd/csrc/pgl_xcorr.hip) against their definition, simulate.lagged_products_host:
the int8 mode bit for bit -- below a tile, across tiles, lags that are no multiples of 4 or 16, rows that are no multiple of 64, K close to
rows, chunks that compose, sums beyond 2^31, the range check that leaves S alone --, the fp64 mode bit for bit on integers and within the
a-priori bound of a sum of `rows` products on real data; then model.simulate(lags=K), its fp64 fallback for counts beyond 127, and
PredictiveCheck(lags=K) against the NumPy path.

The shapes follow the launch plan that lag_i8 derives from them as well as the tile edges (DESIGN.md section 12 has the table): lag groups
past the first (K > 64, up to PGL_LAG_MAX), a workgroup that walks several 512-bin slabs with the plain and with the atomic accumulate (R
taken from the device's compute units, each test asserting that its shape still reaches the path), ldy > N, replicate blocks further apart
than their rows, S blocks further apart than K N N, and first chunks shorter than a lag.  Every call through _device_products also checks
that nothing was written behind `work` or between the blocks of S."""
import functools

import numpy as np
import pytest

from pyglm_amd import simulate
from pyglm_amd.models import NonlinearAutoregressiveModel
from pyglm_amd.regression import (SparseBernoulliRegression, SparseBinomialRegression, SparseGaussianRegression,
                                  SparseNegativeBinomialRegression)
from pyglm_amd.utils.basis import cosine_basis

pytestmark = pytest.mark.gpu

I8, F64 = simulate.LAG_I8, simulate.LAG_F64
SHAPES = [(4, 1, 100), (12, 17, 1000), (20, 5, 333), (70, 33, 2049), (16, 64, 70)]      # (N, K, rows)


WORK_TAIL = 4096                  # bytes of 0xA5 behind the `work` of every call: they must survive it


def _device_products(Y, K, mode, cuts=None, S0=None, ldy=None, pad_rows=(0, 0), col0=0, strideS=None, calls=None):
    """pgl_lagged_products on Y (R, T, N), as one call or cut into the chunks `cuts` (accumulate = 1 after the first, or from the start on a
    given S0) -> (S (R, K, N, N), status (4,)) as NumPy arrays.  `calls`: stop after that many chunks.
    ldy > N: Y is the column window [col0, col0 + N) of rows of ldy doubles; pad_rows = (a, b): every replicate block has a rows in front of
    its T rows and b behind; the cells that are no part of Y hold 1e6.  strideS > K N N: the blocks of S lie that far apart, the gaps hold NaN
    and are asserted to hold it afterwards, as the WORK_TAIL bytes behind every `work` are asserted to be unchanged."""
    import torch
    from pyglm_amd._lib import call, load, ptr
    R, T, N = Y.shape
    ldy = N if ldy is None else ldy
    front, behind = pad_rows
    if ldy == N and front == 0 and behind == 0:
        Y_d = torch.from_numpy(np.array(Y, dtype=np.float64)).cuda()
    else:
        assert col0 + N <= ldy
        wide = np.full((R, front + T + behind, ldy), 1e6)
        wide[:, front:front + T, col0:col0 + N] = Y
        Y_d = torch.from_numpy(wide).cuda()[:, front:front + T, col0:col0 + N]
    strideY = (front + T + behind) * ldy
    block = K * N * N
    strideS = block if strideS is None else strideS
    S_all = torch.full((R, strideS), float("nan"), dtype=torch.float64, device="cuda")
    S = S_all[:, :block]
    if S0 is not None:
        S.copy_(torch.from_numpy(S0.reshape(R, block)))
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    done, works = 0, []
    for rows in (cuts or [T])[:calls]:
        nbytes = load().pgl_lagged_work_bytes(N, K, R, rows)
        work = torch.empty(nbytes + WORK_TAIL, dtype=torch.uint8, device="cuda")
        work[nbytes:] = 0xA5
        works.append(work[nbytes:])
        call("pgl_lagged_products", ptr(Y_d[0, done:]), ldy, strideY, rows, min(K - 1, done), N, K, R, ptr(S_all), strideS,
             1 if (done or S0 is not None) else 0, mode, ptr(work), ptr(status), None)
        done += rows
    assert done == T or calls is not None
    torch.cuda.synchronize()
    assert all(bool((tail == 0xA5).all()) for tail in works), "bytes behind `work` were written"
    assert bool(torch.isnan(S_all[:, block:]).all()), "the gaps between the blocks of S were written"
    return S.cpu().numpy().reshape(R, K, N, N), status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _int_case(N, K, rows, R):
    """int8 inputs over the whole range and their lagged products by the definition"""
    rng = np.random.default_rng(N * 1000 + K + rows + R)
    Y = rng.integers(-127, 128, size=(R, rows, N)).astype(np.float64)
    Y[0, 0, 0], Y[-1, -1, -1] = -127.0, 127.0
    Y.setflags(write=False)
    ref = np.stack([simulate.lagged_products_host(Y[r], K) for r in range(R)])
    ref.setflags(write=False)
    return Y, ref


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N,K,rows", SHAPES)
def test_int8_mode_is_the_definition_bit_for_bit(N, K, rows, R):
    Y, ref = _int_case(N, K, rows, R)
    S, status = _device_products(Y, K, I8)
    assert status[0] == 0
    assert np.array_equal(S, ref)


def test_int8_chunks_compose_to_the_whole_series():
    N, K, rows = 70, 33, 2049
    Y, ref = _int_case(N, K, rows, 3)
    S, status = _device_products(Y, K, I8, cuts=[700, 1, 1348])
    assert status[0] == 0 and np.array_equal(S, ref)
    # and onto sums that are already there
    S0 = np.random.default_rng(1).integers(-1000, 1000, size=ref.shape).astype(np.float64)
    S, _ = _device_products(Y, K, I8, S0=S0)
    assert np.array_equal(S, S0 + ref)


def test_int8_sums_beyond_the_int32_range_are_exact():
    N, K, rows = 16, 2, 140000
    S, status = _device_products(np.full((1, rows, N), 127.0), K, I8)
    assert status[0] == 0 and 127 * 127 * rows > 2 ** 31
    for l in range(K):
        want = 127 * 127 * (rows - l)
        assert all(int(v) == want and v == float(want) for v in S[0, l].ravel())


@pytest.mark.parametrize("bad", [128.0, 0.5, -128.0, float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 127.00000000000001])
def test_int8_mode_refuses_what_is_no_int8_and_leaves_S_alone(bad):
    N, K, rows, R = 20, 5, 333, 3
    Yc, ref = _int_case(N, K, rows, R)
    Y = Yc.copy()
    Y[1, 200, 13] = bad
    S0 = np.random.default_rng(2).standard_normal(ref.shape)
    for given in (S0, None):                                  # accumulate = 1 onto S0; accumulate = 0 onto the NaN fill
        S, status = _device_products(Y, K, I8, S0=given)
        assert list(status) == [3, 200, 1, 13]
        assert np.array_equal(S, S0) if given is not None else np.all(np.isnan(S))
    # the next valid call works, and the fp64 mode takes the refused array (a NaN aside)
    S, status = _device_products(Yc, K, I8)
    assert status[0] == 0 and np.array_equal(S, ref)
    if bad == 128.0 or bad == -128.0:
        S, status = _device_products(Y, K, F64)
        assert status[0] == 0 and np.array_equal(S, np.stack([simulate.lagged_products_host(Y[r], K) for r in range(R)]))


def test_int8_mode_names_one_of_several_values_that_are_no_int8():
    N, K, rows, R = 20, 5, 333, 3
    Yc, ref = _int_case(N, K, rows, R)
    Y = Yc.copy()
    bad = {(0, 311, 19): 200.0, (1, 64, 0): -0.25, (2, 5, 16): float("nan")}          # (replicate, row, neuron)
    for (r, t, n), v in bad.items():
        Y[r, t, n] = v
    S0 = np.random.default_rng(3).standard_normal(ref.shape)
    for given in (S0, None):
        S, status = _device_products(Y, K, I8, S0=given)
        assert status[0] == 3 and (int(status[2]), int(status[1]), int(status[3])) in bad
        assert np.array_equal(S, S0) if given is not None else np.all(np.isnan(S))


# ---- lag groups past the first: K > 64 (L0 > 0, F = lag_front(K) > 64, `l < K` inside a wave's 16 lags, waves that only stage)
LONG_LAGS = [(20, 65, 333, 1), (12, 100, 1000, 3), (16, 128, 300, 1), (20, 129, 700, 2), (8, 256, 600, 2), (4, 256, 256, 1)]   # (N, K, rows, R)
LONG_CUTS = [(12, 100, 1000, 3, [40, 1, 200, 759]), (20, 129, 700, 2, [64, 65, 571])]      # `prev` takes 0, 40, 41, 99 / 0, 64, 128


@pytest.mark.parametrize("N,K,rows,R", LONG_LAGS)
def test_int8_mode_with_more_than_one_lag_group_is_the_definition_bit_for_bit(N, K, rows, R):
    Y, ref = _int_case(N, K, rows, R)
    S, status = _device_products(Y, K, I8)
    assert status[0] == 0
    assert np.array_equal(S, ref)


@pytest.mark.parametrize("N,K,rows,R,cuts", LONG_CUTS)
def test_int8_chunks_compose_with_more_than_one_lag_group(N, K, rows, R, cuts):
    Y, ref = _int_case(N, K, rows, R)
    assert sum(cuts) == rows
    S, status = _device_products(Y, K, I8, cuts=cuts)
    assert status[0] == 0 and np.array_equal(S, ref)
    S0 = np.random.default_rng(K).integers(-1000, 1000, size=ref.shape).astype(np.float64)
    S, status = _device_products(Y, K, I8, cuts=cuts, S0=S0)
    assert status[0] == 0 and np.array_equal(S, S0 + ref)


# ---- a workgroup that walks several slabs of 512 bins: what the plan does once pairs x lag groups x replicates fill the chip.  N = 64 is
# 16 tile pairs, K = 70 two lag groups: 32 workgroups per replicate and time split; R follows the compute units of the device.
def _compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_int8_slab_loop_with_the_plain_accumulate_is_the_definition_bit_for_bit():
    N, K, rows = 64, 70, 1100
    C = _compute_units()
    R = -(-2 * C // 32)
    assert 16 * 2 * R >= 2 * C and rows > 2 * 512         # two workgroups per compute unit without a time split: slabs of 512, 512 and 128 bins
    Y, ref = _int_case(N, K, rows, R)
    S, status = _device_products(Y, K, I8)
    assert status[0] == 0 and np.array_equal(S, ref)
    S, status = _device_products(Y, K, I8, cuts=[600, 500])
    assert status[0] == 0 and np.array_equal(S, ref)
    S0 = np.random.default_rng(4).integers(-1000, 1000, size=ref.shape).astype(np.float64)
    S, status = _device_products(Y, K, I8, S0=S0)
    assert status[0] == 0 and np.array_equal(S, S0 + ref)


def test_int8_slab_loop_with_atomic_adds_is_the_definition_bit_for_bit():
    N, K, rows = 64, 70, 2500
    C = _compute_units()
    R = -(-C // 32)
    rows64 = -(-rows // 64) * 64
    assert -(-2 * C // (32 * R)) < -(-rows64 // 512)      # fewer time splits than slabs: a split spans several (two of 1280 bins at 256 units)
    Y, ref = _int_case(N, K, rows, R)
    S, status = _device_products(Y, K, I8)
    assert status[0] == 0 and np.array_equal(S, ref)


# ---- the layouts the ABI allows besides the packed one
def _f64_int_case(N, K, rows, R):
    """integers beyond the int8 range, whose lagged products the fp64 mode must give exactly, and these by the definition"""
    Y = np.random.default_rng(rows + K).integers(-3000, 3000, size=(R, rows, N)).astype(np.float64)
    return Y, np.stack([simulate.lagged_products_host(Y[r], K) for r in range(R)])


STRIDED = [(20, 5, 333, 3), (20, 65, 333, 2)]               # (N, K, rows, R)


@pytest.mark.parametrize("mode", [I8, F64])
@pytest.mark.parametrize("N,K,rows,R", STRIDED)
def test_rows_and_replicates_further_apart_than_packed(N, K, rows, R, mode):
    # the window [3, 3 + N) of rows of N + 7 doubles, 5 more rows per replicate block (2 in front, 3 behind); every other cell holds 1e6: read
    # by the int8 mode it would set status 3, by the fp64 mode it would spoil the sums
    Y, ref = _int_case(N, K, rows, R) if mode == I8 else _f64_int_case(N, K, rows, R)
    for cuts in (None, [100, 1, 232]):
        S, status = _device_products(Y, K, mode, cuts=cuts, ldy=N + 7, pad_rows=(2, 3), col0=3)
        assert list(status) == [0, 0, 0, 0] and np.array_equal(S, ref)


@pytest.mark.parametrize("mode", [I8, F64])
@pytest.mark.parametrize("N,K,rows,R", STRIDED)
def test_blocks_of_S_further_apart_than_packed(N, K, rows, R, mode):
    # (the helper asserts that the 11 doubles behind every block still hold their NaN)
    Y, ref = _int_case(N, K, rows, R) if mode == I8 else _f64_int_case(N, K, rows, R)
    strideS = K * N * N + 11
    S, status = _device_products(Y, K, mode, strideS=strideS)
    assert status[0] == 0 and np.array_equal(S, ref)
    S0 = np.random.default_rng(5).integers(-1000, 1000, size=ref.shape).astype(np.float64)
    S, status = _device_products(Y, K, mode, S0=S0, strideS=strideS)
    assert status[0] == 0 and np.array_equal(S, S0 + ref)
    S, status = _device_products(Y, K, mode, cuts=[100, 1, 232], strideS=strideS, ldy=N + 7, pad_rows=(2, 3), col0=3)
    assert status[0] == 0 and np.array_equal(S, ref)
    if mode == I8:                                            # refused: S and the gaps as they were
        bad = Y.copy()
        bad[R - 1, 300, 17] = 128.0
        for given in (S0, None):
            S, status = _device_products(bad, K, I8, S0=given, strideS=strideS)
            assert list(status) == [3, 300, R - 1, 17]
            assert np.array_equal(S, S0) if given is not None else np.all(np.isnan(S))


# ---- a first chunk shorter than a lag
SHORT_FIRST = [(12, 17, 1000), (21, 5, 333)]


def _short_cuts(rows):
    return [3, 1, 2, rows - 6]


@pytest.mark.parametrize("N,K,rows", SHORT_FIRST)
def test_int8_chunks_compose_from_a_first_chunk_shorter_than_a_lag(N, K, rows):
    Y, ref = _int_case(N, K, rows, 2)
    S, status = _device_products(Y, K, I8, cuts=_short_cuts(rows))
    assert status[0] == 0 and np.array_equal(S, ref)


@pytest.mark.parametrize("N,K,rows", [(12, 17, 1000), (21, 5, 333), (70, 33, 2049)])
def test_fp64_mode_is_exact_on_integers(N, K, rows):
    rng = np.random.default_rng(rows)
    Y = rng.integers(-3000, 3000, size=(2, rows, N)).astype(np.float64)
    ref = np.stack([simulate.lagged_products_host(Y[r], K) for r in range(2)])
    S, status = _device_products(Y, K, F64)
    assert status[0] == 0 and np.abs(Y).max() > 127 and np.array_equal(S, ref)
    S, _ = _device_products(Y, K, F64, cuts=[rows // 3, 1, rows - rows // 3 - 1])
    assert np.array_equal(S, ref)


def _longdouble_products(Y, K):
    """(the lagged products of Y (T, N) in np.longdouble, those of |Y|)"""
    Yl = np.asarray(Y, dtype=np.longdouble)
    T = Yl.shape[0]
    ref = np.stack([Yl[:T - l].T @ Yl[l:] for l in range(K)])
    mag = np.stack([np.abs(Yl[:T - l]).T @ np.abs(Yl[l:]) for l in range(K)])
    return ref, mag


def _assert_within_summation_bound(S, Y, K):
    """|S - S_ref| <= (rows + 1) 2^-53 sum |y_i y_j|, cell by cell: the a-priori bound of a sum of `rows` products in any order"""
    ref, mag = _longdouble_products(Y, K)
    err = np.abs(S.astype(np.longdouble) - ref)
    bound = (Y.shape[0] + 1) * np.longdouble(2.0) ** -53 * mag
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("N,K,rows", [(12, 17, 1000), (70, 33, 2049)])
def test_fp64_mode_on_real_data_is_within_the_summation_bound(N, K, rows):
    Y = np.random.default_rng(N).standard_normal((1, rows, N))
    S, status = _device_products(Y, K, F64)
    assert status[0] == 0
    _assert_within_summation_bound(S[0], Y[0], K)
    S, _ = _device_products(Y, K, F64, cuts=[rows // 2, rows - rows // 2])
    _assert_within_summation_bound(S[0], Y[0], K)


@pytest.mark.parametrize("N,K,rows,cuts", [(N, K, rows, cuts) for N, K, rows, _, cuts in LONG_CUTS])
def test_fp64_mode_is_exact_on_integers_with_more_than_64_lags(N, K, rows, cuts):
    Y, ref = _f64_int_case(N, K, rows, 2)
    S, status = _device_products(Y, K, F64)
    assert status[0] == 0 and np.abs(Y).max() > 127 and np.array_equal(S, ref)
    S, _ = _device_products(Y, K, F64, cuts=cuts)
    assert np.array_equal(S, ref)


@pytest.mark.parametrize("N,K,rows", SHORT_FIRST)
def test_fp64_chunks_compose_from_a_first_chunk_shorter_than_a_lag(N, K, rows):
    # rows = 3 < K and accumulate = 0: the lags l >= 3 have no product in the first call, and their blocks of S, NaN before it, must become zero
    Y, ref = _f64_int_case(N, K, rows, 2)
    cuts = _short_cuts(rows)
    S, status = _device_products(Y, K, F64, cuts=cuts, calls=1)
    assert status[0] == 0 and np.all(S[:, 3:] == 0.0)
    assert np.array_equal(S[:, :3], np.stack([simulate.lagged_products_host(Y[r, :3], 3) for r in range(2)]))
    S, status = _device_products(Y, K, F64, cuts=cuts)
    assert status[0] == 0 and np.array_equal(S, ref)
    Yr = np.random.default_rng(N + K).standard_normal((1, rows, N))
    S, status = _device_products(Yr, K, F64, cuts=cuts)
    assert status[0] == 0
    _assert_within_summation_bound(S[0], Yr[0], K)


# ---- the model
_MAKE = {
    "bernoulli": lambda N, B, i: SparseBernoulliRegression(N, B, mu_b=-2.0, S_b=0.1),
    "negbin": lambda N, B, i: SparseNegativeBinomialRegression(N, B, xi=(1.0, 2.5)[i % 2], mu_b=-1.0, S_b=0.1),
    "binomial": lambda N, B, i: SparseBinomialRegression(N, B, n=(1, 10, 64)[i % 3], mu_b=-1.0, S_b=0.1),
    "gaussian": lambda N, B, i: SparseGaussianRegression(N, B, eta=(0.3, 0.05)[i % 2], mu_b=0.0, S_b=0.1),
}


def _model(N, B, L, kinds, seed, w_scale=None):
    """a model whose neuron i is of kind kinds[i % len(kinds)], at a random sparse state"""
    np.random.seed(seed)
    regs = [_MAKE[kinds[i % len(kinds)]](N, B, i) for i in range(N)]
    model = NonlinearAutoregressiveModel(N, regs, basis=cosine_basis(B, L=L) / L)
    A, W, b = model._adopt_state()
    rng = np.random.default_rng(seed)
    A[...] = rng.random((N, N)) < 0.5
    W[...] = rng.standard_normal(W.shape) * (w_scale if w_scale is not None else 0.5 / np.sqrt(N))
    W /= np.array([getattr(r, "n", 4.0 if hasattr(r, "xi") else 1.0) for r in regs], dtype=float)[None, :, None]   # counts weigh as spikes do
    base = {"bernoulli": -2.0, "negbin": -0.5, "binomial": -1.0, "gaussian": 0.1}
    b[:, 0] = [base[kinds[i % len(kinds)]] for i in range(N)] + 0.3 * rng.standard_normal(N)
    return model


MODELS = [(12, 3, 30, ("bernoulli", "binomial"), 3, 2000, 20), (64, 5, 100, ("bernoulli",), 8, 1500, 50),
          (12, 3, 30, ("bernoulli", "binomial"), 3, 2000, 100)]                          # the last: two lag groups


@functools.lru_cache(maxsize=None)
def _model_case(case):
    """the model of MODELS[case] and its simulation on the NumPy path, lagged products included"""
    N, B, L, kinds, R, T, K = MODELS[case]
    model = _model(N, B, L, kinds, seed=N + R)
    host = model.simulate(T, replicates=R, seed=500 + N, gpu=False, lags=K)
    for a in (host.Y, host.lagged):
        a.setflags(write=False)
    return model, host


@pytest.mark.parametrize("case", range(len(MODELS)))
def test_simulate_on_the_device_folds_the_lagged_products_of_its_paths(case):
    N, B, L, kinds, R, T, K = MODELS[case]
    model, host = _model_case(case)
    sim = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K)
    assert sim.lagged.shape == (R, K, N, N) and sim.lag_redos == 0 and sim.Y.sum() > 0
    for r in range(R):
        assert np.array_equal(sim.lagged[r], simulate.lagged_products_host(sim.Y[r], K))
    assert np.array_equal(sim.Y, host.Y) and np.array_equal(sim.lagged, host.lagged)
    assert np.array_equal(sim.correlogram(), host.correlogram(), equal_nan=True)
    bare = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K, keep_paths=False)
    assert bare.Y is None and np.array_equal(bare.lagged, host.lagged) and np.array_equal(bare.history, host.history)
    plain = model.simulate(T, replicates=R, seed=500 + N, gpu=True)
    assert plain.lagged is None and np.array_equal(plain.Y, host.Y)


@pytest.mark.parametrize("case,chunk", [(0, 7), (0, 300), (1, 37), (1, 400), (2, 37)])
def test_simulate_folds_the_same_sums_whatever_the_chunks(case, chunk, monkeypatch):
    # 7 < K - 1 = 19, 37 < K - 1 = 49 and 37 < K - 1 = 99: a chunk shorter than the rows kept before it; none of the five divides T
    N, B, L, kinds, R, T, K = MODELS[case]
    model, host = _model_case(case)
    assert T % chunk != 0
    monkeypatch.setattr(simulate, "chunk_bins", lambda N, B, R=1: chunk)
    for keep in (True, False):
        sim = model.simulate(T, replicates=R, seed=500 + N, gpu=True, lags=K, keep_paths=keep)
        assert np.array_equal(sim.lagged, host.lagged) and np.array_equal(sim.sum, host.sum)


def test_counts_beyond_127_are_folded_in_fp64():
    N, B, L, R, T, K = 12, 3, 30, 3, 600, 20
    model = _model(N, B, L, ("negbin",), seed=41, w_scale=0.02 / np.sqrt(N))
    model._adopt_state()[2][:, 0] = 3.0 + 0.1 * np.random.default_rng(42).standard_normal(N)
    before = simulate.LAG_REDOS
    sim = model.simulate(T, replicates=R, seed=43, gpu=True, lags=K)
    assert sim.Y.max() > 127
    assert sim.lag_redos > 0 and simulate.LAG_REDOS == before + sim.lag_redos
    for r in range(R):
        assert np.array_equal(sim.lagged[r], simulate.lagged_products_host(sim.Y[r], K))
    host = model.simulate(T, replicates=R, seed=43, gpu=False, lags=K)
    assert np.array_equal(sim.Y, host.Y) and np.array_equal(sim.lagged, host.lagged)
    # a count model that stays below 128 never leaves the int8 kernel
    calm = _model(N, B, L, ("negbin",), seed=41, w_scale=0.02 / np.sqrt(N))
    low = calm.simulate(T, replicates=R, seed=43, gpu=True, lags=K)
    assert low.Y.max() <= 127 and low.lag_redos == 0
    assert np.array_equal(low.lagged[0], simulate.lagged_products_host(low.Y[0], K))


def test_a_gaussian_model_is_folded_in_fp64_within_the_summation_bound():
    N, B, L, R, T, K = 12, 3, 30, 2, 1500, 20
    model = _model(N, B, L, ("gaussian", "bernoulli"), seed=31, w_scale=0.5 / np.sqrt(N * B))
    sim = model.simulate(T, replicates=R, seed=32, gpu=True, lags=K)
    assert np.std(sim.Y) > 0.1 and sim.lag_redos == 0
    for r in range(R):
        _assert_within_summation_bound(sim.lagged[r], sim.Y[r], K)
    host = model.simulate(T, replicates=R, seed=32, gpu=False, lags=K)
    np.testing.assert_allclose(sim.lagged, host.lagged, rtol=1e-9, atol=1e-9)        # (the two paths' Y agree to 1e-10: test_gpu_simulate.py)


def test_memory_for_the_lagged_products_is_checked_before_allocating():
    from pyglm_amd._lib import PglError
    N, R, K = 4096, 16, 256                                     # 512 GiB of sums
    with pytest.raises(PglError) as err:
        simulate.simulate(np.zeros((N, N)), np.zeros(N), np.ones((2, 1)), np.zeros(N, dtype=np.int32), np.zeros(N), 1000, replicates=R, seed=1,
                          keep_paths=False, on_device=True, lags=K)
    assert "lags" in str(err.value) and "replicates" in str(err.value)


def test_cross_correlogram_of_a_data_set():
    model = _model(12, 3, 30, ("bernoulli", "binomial"), seed=51)
    data = model.simulate(1200, seed=52, gpu=False).Y[0]
    model.add_data(data)
    d, h = model.cross_correlogram(lags=15, gpu=True), model.cross_correlogram(lags=15, gpu=False)
    assert d.shape == (15, 12, 12) and np.array_equal(d, h, equal_nan=True) and np.isfinite(d).any()


def test_cross_correlogram_of_a_data_set_with_three_lag_groups():
    model = _model(12, 3, 30, ("bernoulli", "binomial"), seed=51)
    model.add_data(model.simulate(1200, seed=52, gpu=False).Y[0])
    d, h = model.cross_correlogram(lags=130, gpu=True), model.cross_correlogram(lags=130, gpu=False)
    assert d.shape == (130, 12, 12) and np.array_equal(d, h, equal_nan=True) and np.isfinite(d).any()


def _predictive_check_matches_the_host_path(K):
    N, R = 12, 4
    model = _model(N, 3, 30, ("bernoulli", "binomial"), seed=61)
    model.add_data(model.simulate(1000, seed=62, gpu=False).Y[0])
    out = []
    for gpu in (True, False):
        ppc = model.predictive_check(replicates=R, seed=63, gpu=gpu, lags=K)
        for _ in range(3):
            ppc.collect()
        out.append(ppc)
    d, h = out
    assert d.observed["xcorr"].shape == (K, N, N) and np.array_equal(d.observed["xcorr"], h.observed["xcorr"], equal_nan=True)
    p = d.pvalue("xcorr")
    assert p.shape == (K, N, N) and np.array_equal(p, h.pvalue("xcorr"), equal_nan=True)
    assert np.nanmin(p) >= 2.0 / 13.0 and len(np.unique(p[~np.isnan(p)])) > 3
    np.testing.assert_allclose(d.xcorr_mean, h.xcorr_mean, rtol=0, atol=1e-12)
    np.testing.assert_allclose(d.xcorr_std, h.xcorr_std, rtol=0, atol=1e-12)
    for stat in ("rate", "fano"):
        assert np.array_equal(d.pvalue(stat), h.pvalue(stat), equal_nan=True)


def test_predictive_check_with_lags_matches_the_host_path():
    _predictive_check_matches_the_host_path(10)


def test_predictive_check_with_two_lag_groups_matches_the_host_path():
    _predictive_check_matches_the_host_path(70)
