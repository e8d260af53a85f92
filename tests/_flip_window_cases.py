"""Inputs and longdouble references of tests/test_gpu_flip_windows.py, built on the host (tests/test_flip_window_cases_host.py builds them
without a GPU and so checks the conditions below there).

One case per block size B: R = pgl_flip_window_blocks(B) from the library, N = 2 R + 3 blocks -- two full proposal windows and a ragged third
of 3 blocks.  J, h = wellcond_system(N B + 1); about half the blocks start active; the initial tableau is the longdouble sweep of
[[J, h], [h', 0]] on {bias} U {active rows} ROUNDED TO FP64: that array is what the device gets and what the reference starts from, so the
device answers for the windows only.  The neurons of a case share all that and differ in perm, u, rho and c0:
    mixed       c0 = -(dml of the block at the initial tableau) + N(0, 1.5^2), rho in (0.3, 0.7) but for four entries that are exactly 0 or 1
    skipped     the mixed neuron's inputs with skip = 1
    nothing     rho = 1/2, c0 shifted by 20 towards the block's current state
    everything  rho = 1/2, c0 shifted by 6 against it: panels of nearly R B rows
Conditions on the inputs, asserted here from the reference alone (a seed that fails one is changed, never the condition):
    |u - threshold| >= 1e-6 at every proposal;  the mixed neuron flips a block on and a block off in each of windows 0 and 1;  the nothing
    neuron flips nothing;  the everything neuron has more than 128 pivot rows in a full window (B <= 16)."""
import numpy as np

from tests import _dense_ref as R

BLOCK_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 11, 16, 32]
KINDS = ["mixed", "skipped", "nothing", "everything"]
MARGIN = 1e-6
SEEDS = {32: 1034}                            # B -> seed, where 1000 + B fails a condition (B = 32: windows of 5 proposals; 1032 and 1033
#                                               leave a window of the mixed neuron without a flip in one of the two directions)


def window_blocks(B):
    from pyglm_amd import _lib
    return _lib.load().pgl_flip_window_blocks(B)


def _windows_of(flips, Rw, nwin):
    out = [[] for _ in range(nwin)]
    for k, m, s in flips:
        out[k // Rw].append((k, m, s))
    return out


def build_case(B, Rw=None):
    """dict(B, R, N, D, Md, nwin, J, h, a0, M0 (fp64), neurons = {kind: dict(perm, u, rho, c0, skip, ref)}) with ref = None for the skipped
    neuron and else flip_proposals' result plus, per window, flips[w] = [(k, m, sign)], kappa[w] = kappa_2 of the window's pivot block as it
    stood before the window (0 for a window without flips)"""
    Rw = window_blocks(B) if Rw is None else Rw
    N = 2 * Rw + 3
    D, Md, nwin = N * B, N * B + 2, 3
    rng = np.random.default_rng(SEEDS.get(B, 1000 + B))
    J, h = R.wellcond_system(D + 1, rng)
    a0 = rng.permutation(N) < (N + 1) // 2
    S0 = np.array([D] + [m * B + b for m in np.nonzero(a0)[0] for b in range(B)])
    M0 = np.asarray(R.sweep(R.tableau(J, h), S0, np.ones(len(S0))), dtype=np.float64)
    M0l = R.ld(M0)
    dml0 = np.array([R.block_dml(M0l, np.arange(m * B, (m + 1) * B), a0[m]) for m in range(N)], dtype=R.LD)
    toward = np.where(a0, 1.0, -1.0)
    neurons = {}
    for kind in KINDS:
        if kind == "skipped":
            neurons[kind] = dict(neurons["mixed"], skip=1, ref=None)
            continue
        perm, u = rng.permutation(N), rng.random(N)
        if kind == "mixed":
            rho = rng.uniform(0.3, 0.7, N)
            c0 = np.asarray(-dml0, dtype=np.float64) + 1.5 * rng.standard_normal(N)
            special = []
            for w, wanted in ((0, [(True, 1.0), (False, 0.0)]), (1, [(True, 0.0), (False, 1.0)])):
                for on, r in wanted:          # the first steps of the window (from its third on, where it is long enough) whose block is in the wanted state
                    k = next(k for k in range(w * Rw + (2 if Rw >= 8 else 0), (w + 1) * Rw) if a0[perm[k]] == on and k not in special)
                    rho[perm[k]] = r
                    special.append(k)
        else:
            rho = np.full(N, 0.5)
            c0 = np.asarray(-dml0, dtype=np.float64) + (20.0 if kind == "nothing" else -6.0) * toward
            special = []
        ref = R.flip_proposals(M0l, a0, perm, u, rho, c0, B, R=Rw)
        ref["special"] = special
        ref["win_flips"] = _windows_of(ref["flips"], Rw, nwin)
        before = [M0l] + [s[0] for s in ref["snaps"][:-1]]
        ref["kappa"] = []
        for w in range(nwin):
            rows = [m * B + b for _, m, _ in ref["win_flips"][w] for b in range(B)]
            ref["kappa"].append(float(np.linalg.cond(np.asarray(before[w][np.ix_(rows, rows)], dtype=np.float64))) if rows else 0.0)
        neurons[kind] = dict(perm=perm, u=u, rho=rho, c0=c0, skip=0, ref=ref)
    case = dict(B=B, R=Rw, N=N, D=D, Md=Md, nwin=nwin, J=J, h=h, a0=a0, M0=M0, neurons=neurons)
    check_conditions(case)
    return case


def check_conditions(case):
    B, Rw = case["B"], case["R"]
    assert len(case["neurons"]["mixed"]["ref"]["snaps"]) == case["nwin"] == -(-case["N"] // Rw)
    for kind in ("mixed", "nothing", "everything"):
        nr = case["neurons"][kind]
        ref = nr["ref"]
        rated = np.array([0 < nr["rho"][m] < 1 for m in nr["perm"]])
        assert np.array_equal(np.isnan(ref["threshold"].astype(float)), ~rated)
        margin = np.abs(R.ld(nr["u"]) - ref["threshold"])[rated]
        assert margin.min() >= MARGIN, "B = %d %s: a proposal within %.1e of its threshold" % (B, kind, float(margin.min()))
    mixed = case["neurons"]["mixed"]
    assert len(mixed["ref"]["special"]) == 4 and sorted(k // Rw for k in mixed["ref"]["special"]) == [0, 0, 1, 1]
    assert sorted((bool(case["a0"][mixed["perm"][k]]), float(mixed["rho"][mixed["perm"][k]])) for k in mixed["ref"]["special"]) == \
        [(False, 0.0), (False, 1.0), (True, 0.0), (True, 1.0)]
    for w in (0, 1):
        signs = [s for _, _, s in mixed["ref"]["win_flips"][w]]
        assert 1 in signs and -1 in signs, "B = %d: the mixed neuron does not flip both ways in window %d" % (B, w)
    assert case["neurons"]["nothing"]["ref"]["flips"] == []
    if B <= 16:
        assert max(len(f) for f in case["neurons"]["everything"]["ref"]["win_flips"][:2]) * B > 128
