"""The longdouble references of tests/_dense_ref.py against their own defining identities, on the CPU: a wrong reference must not be able to
pass for a wrong kernel.  (np.longdouble is the 80-bit x87 type on the machines this suite runs on, eps 1.08e-19, as tests/test_gpu_i8gram.py
already relies on; the identities below are asserted at 1e-15 or tighter, which fp64 arithmetic could not meet at these sizes.)"""
import numpy as np
import pytest

from tests import _dense_ref as R

LD = np.longdouble


def _rel(a, b):
    return float(np.max(np.abs(R.ld(a) - R.ld(b))) / np.max(np.abs(R.ld(b))))


@pytest.fixture(scope="module")
def system():
    """a 62-row posterior in the tableau's layout: 15 blocks of 4, the bias row last; kappa_2 about 3.6"""
    rng = np.random.default_rng(11)
    J, h = R.wellcond_system(61, rng)
    return J, h, R.tableau(J, h)


def test_longdouble_is_wider_than_fp64():
    assert np.finfo(LD).eps < 2e-19


@pytest.mark.parametrize("n", [1, 2, 47, 48, 49, 97, 150])
def test_chol_upper_reproduces_the_matrix(n):
    rng = np.random.default_rng(n)
    for J, _ in (R.wellcond_system(n, rng), R.spectrum_system(n, 1e6, rng)):
        U = R.chol_upper(J)
        assert U.dtype == LD and np.array_equal(U, np.triu(U)) and np.all(np.diag(U) > 0)
        assert _rel(U.T @ U, J) < 1e-17
        # only the upper triangle is read
        assert np.array_equal(R.chol_upper(np.triu(J)), U)


def test_chol_upper_refuses_an_indefinite_matrix():
    J, _ = R.wellcond_system(20, np.random.default_rng(0))
    J[7, 7] = -J[7, 7]
    with pytest.raises(np.linalg.LinAlgError):
        R.chol_upper(J)


def test_draw_is_the_law_of_sample_gaussian():
    rng = np.random.default_rng(5)
    for J, h in (R.wellcond_system(90, rng), R.spectrum_system(90, 1e6, rng)):
        z = rng.standard_normal(90)
        mu, x = R.draw(J, h, z)
        U = R.chol_upper(J)
        kappa = np.linalg.cond(J)
        assert _rel(R.ld(J) @ mu, h) < 1e-18 * kappa
        assert _rel(U @ (x - mu), z) < 1e-18 * kappa
        # against fp64 LAPACK, to fp64's own accuracy
        L = np.linalg.cholesky(J)
        np.testing.assert_allclose(np.asarray(x, dtype=float), np.linalg.solve(J, h) + np.linalg.solve(L.T, z), rtol=0,
                                   atol=1e-14 * kappa * float(np.max(np.abs(x))))


def test_one_factorisation_serves_every_nested_prefix():
    rng = np.random.default_rng(6)
    J, _ = R.wellcond_system(81, rng)
    D = 80
    U_full = R.chol_upper(J[:D, :D])
    w_full = R.solve_upper_t(U_full, J[:D, D])
    for k in (0, 1, 37, 48, 80):
        ix = list(range(k)) + [D]
        assert _rel(R.bordered_prefix_factor(U_full, w_full, J[D, D], k), R.chol_upper(J[np.ix_(ix, ix)])) < 1e-17


def test_tableau_definition_on_a_bias_first_list(system):
    J, h, A = system
    D, B = 60, 4
    blocks = [1, 4, 5, 9, 14]
    S = np.array([D] + [m * B + b for m in blocks for b in range(B)])
    M = R.sweep(A, S, np.ones(len(S)))
    P = R.inv_sym(J[np.ix_(S, S)])
    assert _rel(R.ld(J[np.ix_(S, S)]) @ P, np.eye(len(S))) < 1e-17
    rest = np.setdiff1d(np.arange(D + 1), S)
    assert _rel(M[np.ix_(S, S)], -P) < 1e-16
    assert _rel(M[S, D + 1], P @ R.ld(h[S])) < 1e-16
    JRS = R.ld(J[np.ix_(rest, S)])
    assert _rel(M[np.ix_(rest, rest)], R.ld(J[np.ix_(rest, rest)]) - JRS @ P @ JRS.T) < 1e-16
    assert _rel(M[rest, D + 1], R.ld(h[rest]) - JRS @ P @ R.ld(h[S])) < 1e-16
    assert _rel(M[D + 1, D + 1], -R.ld(h[S]) @ P @ R.ld(h[S])) < 1e-16
    assert _rel(M, M.T) < 1e-18


def test_forward_then_reverse_gives_the_input_back(system):
    _, _, A = system
    S = np.array([60, 8, 9, 10, 11, 40, 41, 42, 43, 0, 1, 2, 3])
    M = R.sweep(R.sweep(A, S, np.ones(len(S))), S, -np.ones(len(S)))
    assert _rel(M, A) < 1e-16


def test_sequential_sweeps_equal_the_block_formula(system):
    _, _, A = system
    rng = np.random.default_rng(2)
    S = np.array([60] + [m * 4 + b for m in (0, 3, 7, 12) for b in range(4)])
    sg = np.ones(len(S))
    M1 = R.sweep(A, S, sg)
    assert _rel(R.sweep_block(A, S, sg), M1) < 1e-16
    assert _rel(R.sweep(A, S[rng.permutation(len(S))], sg), M1) < 1e-16          # the order of the pivots does not matter
    # a mixed list on the swept tableau: reverse two of the blocks, forward two new ones
    D2 = np.array([m * 4 + b for m in (3, 12, 5, 9) for b in range(4)])
    sg2 = np.repeat([-1.0, -1.0, 1.0, 1.0], 4)
    assert _rel(R.sweep_block(M1, D2, sg2), R.sweep(M1, D2, sg2)) < 1e-16


def test_a_mixed_list_equals_the_sweep_of_the_net_set(system):
    _, _, A = system
    S = np.array([60] + [m * 4 + b for m in (0, 3, 7, 12) for b in range(4)])
    M1 = R.sweep(A, S, np.ones(len(S)))
    D2 = np.array([m * 4 + b for m in (3, 12, 5, 9) for b in range(4)])
    sg2 = np.repeat([-1.0, -1.0, 1.0, 1.0], 4)
    net = np.array([60] + [m * 4 + b for m in (0, 5, 7, 9) for b in range(4)])
    assert _rel(R.sweep(M1, D2, sg2), R.sweep(A, net, np.ones(len(net)))) < 1e-15


def test_scaling_the_tableau_by_a_power_of_two_scales_the_swept_tableau_exactly(system):
    _, _, A = system
    S = np.array([60] + [m * 4 + b for m in (2, 3, 11) for b in range(4)])[:11]       # a list cut inside a block, as a chunk border does
    M = R.sweep(A, S, np.ones(len(S)))
    for c in (0.25, 8.0):
        assert np.array_equal(R.scale_swept(M, S, c), R.sweep(A * R.LD(c), S, np.ones(len(S))))
    assert np.array_equal(R.scale_swept(A, [], 4.0), A * 4)


# ---------------------------------------------------------------------------------------------------------------- the collapsed proposals
def _swept_on_active(J, h, a, B):
    D = len(a) * B
    S = np.array([D] + [m * B + b for m in np.nonzero(a)[0] for b in range(B)])
    return R.sweep(R.tableau(J, h), S, np.ones(len(S)))


def _dense_marginal(J, h, c0, a, B):
    """-1/2 log|J_SS| + 1/2 h_S' J_SS^-1 h_S + sum of c0 over the active blocks, S = {bias} U {active blocks}, by a Cholesky of J_SS"""
    D = len(a) * B
    S = np.array([m * B + b for m in np.nonzero(a)[0] for b in range(B)] + [D], dtype=int)
    U = R.chol_upper(J[np.ix_(S, S)])
    w = R.solve_upper_t(U, h[S])
    return -np.sum(np.log(np.diag(U))) + (w @ w) / 2 + np.sum(R.ld(c0)[np.asarray(a, dtype=bool)])


def test_flip_logodds_telescope_to_the_dense_marginal_likelihood():
    """N = 6, B = 3, rho = 1/2 (no prior odds): the log-odds of the steps that flip, signed by the direction, add up to the difference of the
    marginal likelihoods of the final and the initial set -- each computed from J itself, without a tableau"""
    N, B = 6, 3
    seen = 0
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        J, h = R.wellcond_system(N * B + 1, rng)
        a0 = rng.random(N) < 0.5
        c0 = rng.standard_normal(N)
        out = R.flip_proposals(_swept_on_active(J, h, a0, B), a0, rng.permutation(N), rng.random(N), np.full(N, 0.5), c0, B)
        total = sum(s * out["logodds"][k] for k, _, s in out["flips"])
        want = _dense_marginal(J, h, c0, out["a"], B) - _dense_marginal(J, h, c0, a0, B)
        # (longdouble: eps 1.1e-19; the terms are of order 1 to 10, a few dozen operations each)
        assert abs(total - want) < 1e-16 * max(1.0, abs(float(want))), (seed, float(total), float(want))
        # the final tableau is the sweep of A on the final set
        assert _rel(out["M"], _swept_on_active(J, h, out["a"], B)) < 1e-15
        seen += len(out["flips"])
    assert seen >= 4


def test_flip_proposals_agree_with_the_fp64_oracle():
    """one small regression problem: the oracle takes two dense Choleskys of the active sub-system per proposal (fp64 LAPACK), the reference
    here reads a B x B block of the swept tableau -- two formulations of the same log-odds, held to the suite's own log-odds tolerance
    (tests/test_gpu_parity.py: _check_logodds).  One rho is exactly 0 and one exactly 1: NaN log-odds and the decision 0 on both sides."""
    from oracle import pyglm_oracle as orc
    N, B, T = 9, 3, 300
    rng = np.random.default_rng(21)
    X = np.abs(rng.standard_normal((T, N, B))) * 0.4
    y = (rng.random(T) < 0.3).astype(float)
    om = rng.gamma(2.0, 0.12, T)
    rho = np.full(N, 0.35)
    perm = rng.permutation(N)
    a0 = rng.random(N) < 0.5
    on, off = perm[2:][a0[perm[2:]]][0], perm[2:][~a0[perm[2:]]][0]
    rho[on], rho[off] = 1.0, 0.0
    r = orc.Regression(N, B, rho=rho, S_w=2.0, mu_w=0.3, mu_b=-0.5, S_b=1.0)
    r.a, r.W, r.b = a0.copy(), np.zeros((N, B)), np.zeros(1)
    u, trace = rng.random(N), []
    J_post, h_post = r.resample([(X, y)], [om], perm, u, rng.standard_normal(N * B + 1), trace=trace)
    J_w, h_w, _, _ = r.natural_params()
    c0 = np.array([0.5 * np.linalg.slogdet(J_w[m])[1] - 0.5 * r.mu_w[m] @ J_w[m] @ r.mu_w[m] for m in range(N)])
    out = R.flip_proposals(_swept_on_active(J_post, h_post, a0, B), a0, perm, u, rho, c0, B)
    want = np.array([t[1] for t in trace])
    assert [t[0] for t in trace] == perm.tolist() and np.array_equal(out["decision"], [t[2] for t in trace])
    assert np.array_equal(np.isnan(want), np.isnan(out["logodds"].astype(float))) and np.isnan(want).sum() == 2
    ok = ~np.isnan(want)
    np.testing.assert_allclose(out["logodds"].astype(float)[ok], want[ok], rtol=1e-10, atol=1e-9)
    assert np.array_equal(out["a"], r.a) and len(out["flips"]) >= 2 and out["decision"][perm.tolist().index(on)] == 0


def test_flip_proposals_do_not_depend_on_the_window_length():
    N, B = 7, 2
    rng = np.random.default_rng(8)
    J, h = R.wellcond_system(N * B + 1, rng)
    a0 = rng.random(N) < 0.5
    args = (_swept_on_active(J, h, a0, B), a0, rng.permutation(N), rng.random(N), rng.uniform(0.2, 0.8, N), rng.standard_normal(N), B)
    base = R.flip_proposals(*args)
    assert base["snaps"] == [] and len(base["flips"]) >= 2
    runs = {r: R.flip_proposals(*args, R=r) for r in (2, 3, 7, 10)}
    for r, out in runs.items():
        for key in ("logodds", "decision", "threshold", "M", "a"):
            assert np.array_equal(out[key], base[key], equal_nan=True), (r, key)
        assert out["flips"] == base["flips"] and len(out["snaps"]) == -(-N // r)
        assert np.array_equal(out["snaps"][-1][0], base["M"]) and np.array_equal(out["snaps"][-1][1], base["a"])
    # the boundary after six steps is the third of R = 2 and the second of R = 3
    assert np.array_equal(runs[2]["snaps"][2][0], runs[3]["snaps"][1][0]) and np.array_equal(runs[2]["snaps"][2][1], runs[3]["snaps"][1][1])
    assert np.array_equal(base["decision"], (R.ld(args[3]) > base["threshold"]).astype(int))      # the threshold is the decision


def test_position_order_puts_block_perm_k_at_position_k():
    B, perm = 2, np.array([2, 0, 1])
    M = np.arange(64.0).reshape(8, 8)
    P = R.position_order(M, perm, B)
    rows = [4, 5, 0, 1, 2, 3, 6, 7]
    assert np.array_equal(P, M[np.ix_(rows, rows)])


def test_inv_spd_and_matrix_right_hand_sides():
    J, _ = R.spectrum_system(70, 1e6, np.random.default_rng(4))
    assert _rel(R.ld(J) @ R.inv_spd(J), np.eye(70)) < 1e-18 * 1e6
    assert _rel(R.inv_spd(J), R.inv_sym(J)) < 1e-18 * 1e6


def test_the_matrix_families_have_the_stated_condition():
    rng = np.random.default_rng(9)
    J, _ = R.wellcond_system(400, rng)
    assert 3.0 < np.linalg.cond(J) < 4.5
    J, _ = R.spectrum_system(129, 1e6, rng)
    assert abs(np.linalg.cond(J) / 1e6 - 1) < 1e-6
    assert R.bound(129, J) == pytest.approx(8 * 129 * 2.0 ** -53 * 1e6, rel=1e-6)


def test_relerr_flags_nan():
    assert R.relerr(np.array([1.0, np.nan]), np.array([1.0, 2.0])) == np.inf
    assert R.relerr(np.array([1.0, 2.0]), np.array([1.0, 2.0])) == 0.0
