"""The tableau update on its own: pgl_flip_apply, pgl_flip_apply_chunk and pgl_flip_visit_order (pgl_flips.hip) through FlipState, against
the longdouble sweeps of tests/_dense_ref.py (checked on the CPU by tests/test_dense_ref_host.py).

What the kernels do: the pivot-block inverse G = M_DD^-1 in LDS (lists of up to 128 rows) or by recursive 2 x 2 blocking of 128-row
in-register inversions on a 256- or 512-row frame padded with the identity (chunks of the initial sweep), then the panel gather, the
rank-k update on the lower-triangular tiles and the fix-up of the pivot rows and columns.  The lists below sit on the edges the code names:
129..256 and 257..512 rows with short neurons riding in the long ones' launches, tiles of the gather / fix-up on either side of the s_min
split, d_cnt = 0, reverse and mixed lists, block rows that do not ascend.

The tableau is A = [[J, h], [h', 0]] of N = 150 blocks of B = 4 (Md = 602).  The pivot lists are what production builds: the bias row D first,
then the rows of whole blocks ascending, cut at the chunk's length.  One reference pass over the longest list gives every prefix of it; the
neurons of a batch carry c_n A for powers of two c_n (tests/_dense_ref.py: scale_swept -- exact), so a kernel that reads a neighbour's tableau
does not pass.

Tolerance: max |M_dev - M_ref| / max |M_ref| over the lower triangle <= 8 Md 2^-53 kappa_2(M_DD) of the pivot block as it stood before the
call; two calls in a row are held to the sum of their two bounds.  Everything else is exact.  Each case prints its measured maximum."""
import ctypes

import numpy as np
import pytest

from tests import _dense_ref as R

pytestmark = pytest.mark.gpu

SENT = -777.25
N, B = 150, 4
D, Md = N * B, N * B + 2
KMAX = 512
BATCHES = {                                   # name -> (max_pivots of pgl_flip_apply_chunk or None for pgl_flip_apply, d_cnt per neuron)
    "apply": (None, [0, 1, 17, 127, 128]),
    "chunk256": (256, [0, 5, 129, 255, 256]),
    "chunk512": (512, [3, 257, 383, 385, 511, 512]),
}
EXTRA_COUNTS = [100, 125, 253, 300, 441]      # two chunks in a row; lists of shuffled blocks
SCALES = [1.0, 4.0, 0.5, 2.0, 0.25, 8.0]


def _ldj():
    from pyglm_amd._lib import call
    v = ctypes.c_int()
    call("pgl_sweep_dims", N, B, 1, None, None, ctypes.byref(v))
    return v.value


def _pack(tabs, ldj):
    """tableaux (Md x Md, any float type) -> (nb, ldj, ldj) fp64: the lower triangle, NaN above it ("lower triangle valid"), a sentinel in
    the padding rows and columns, which nothing may write"""
    out = np.full((len(tabs), ldj, ldj), SENT)
    il, iu = np.tril_indices(Md), np.triu_indices(Md, 1)
    for n, A in enumerate(tabs):
        out[n][il] = np.asarray(A, dtype=np.float64)[il]
        out[n][iu] = np.nan
    return out


def _apply(Mh, lists, max_pivots=None, calls=1):
    """Mh (nb, ldj, ldj) host; lists: per neuron (idx, sign), or per call a list of those.  Scratch is NaN, batch_k a sentinel."""
    import torch
    from pyglm_amd._lib import FlipState, call
    dev = torch.device("cuda:0")
    nb, ldj = Mh.shape[0], Mh.shape[1]
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    M = torch.from_numpy(Mh).to(dev)
    G = torch.full((nb, KMAX, KMAX), float("nan"), **f64)
    Lws = torch.full((nb, (KMAX + 1) ** 2), float("nan"), **f64)
    Ut, Wt = torch.full((nb, KMAX, ldj), float("nan"), **f64), torch.full((nb, KMAX, ldj), float("nan"), **f64)
    status, batch_k = torch.zeros(nb, **i32), torch.full((nb,), -7, **i32)
    d_idx, d_sign, d_cnt = torch.zeros(nb, KMAX, **i32), torch.full((nb, KMAX), float("nan"), **f64), torch.zeros(nb, **i32)
    s = FlipState(M=M.data_ptr(), ldj=ldj, strideM=ldj * ldj, nb=nb, N=N, B=B, d_idx=d_idx.data_ptr(), d_sign=d_sign.data_ptr(),
                  d_cnt=d_cnt.data_ptr(), batch_k=batch_k.data_ptr(), G=G.data_ptr(), Lws=Lws.data_ptr(), Ut=Ut.data_ptr(), Wt=Wt.data_ptr(),
                  ldu=ldj, status=status.data_ptr(), visit_order=0)
    per_call = lists if calls > 1 else [lists]
    mp = max_pivots if isinstance(max_pivots, (list, tuple)) else [max_pivots] * len(per_call)
    snaps = []
    for ls, m in zip(per_call, mp):
        ih, sh, ch = np.zeros((nb, KMAX), dtype=np.int32), np.full((nb, KMAX), np.nan), np.zeros(nb, dtype=np.int32)
        for n, (idx, sg) in enumerate(ls):
            assert len(idx) <= (m or 128) and (len(idx) == 0 or (0 <= min(idx) and max(idx) <= D)), "never the potential row, never out of range"
            ih[n, :len(idx)], sh[n, :len(idx)], ch[n] = idx, sg, len(idx)
        d_idx.copy_(torch.from_numpy(ih)); d_sign.copy_(torch.from_numpy(sh)); d_cnt.copy_(torch.from_numpy(ch))
        if m is None:
            call("pgl_flip_apply", ctypes.byref(s), None)
        else:
            call("pgl_flip_apply_chunk", ctypes.byref(s), m, None)
        torch.cuda.synchronize()
        snaps.append(dict(M=M.cpu().numpy(), status=status.cpu().numpy(), batch_k=batch_k.cpu().numpy(), G=G.cpu().numpy()))
    return snaps if calls > 1 else snaps[0]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _lower_err(Mdev, ref):
    il = np.tril_indices(Md)
    return R.relerr(Mdev[:Md, :Md][il], ref[il])


def _padding_untouched(Mdev):
    return bool(np.all(Mdev[Md:, :] == SENT) and np.all(Mdev[:, Md:] == SENT))


def _rows(blocks):
    return [int(m) * B + b for m in blocks for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------- the shared reference
@pytest.fixture(scope="module")
def master():
    """one posterior (kappa_2 about 3.6), one production list of 512 rows (bias, then 128 scattered blocks ascending, the first and the last
    block among them), one longdouble pass over it with a copy kept at every length the tests use"""
    rng = np.random.default_rng(4242)
    J, h = R.wellcond_system(D + 1, rng)
    A = R.tableau(J, h)
    blocks = np.sort(np.concatenate([[0, N - 1], 1 + rng.choice(N - 2, 126, replace=False)]))
    lst = np.array([D] + _rows(blocks))[:KMAX]
    counts = sorted(set(k for _, cs in BATCHES.values() for k in cs) | set(EXTRA_COUNTS))
    swept = R.sweep_prefixes(A, lst, np.ones(len(lst)), counts)
    return dict(J=J, h=h, A=A, list=lst, blocks=blocks, swept=swept, ldj=_ldj())


def _bound(master, k, lst=None):
    lst = master["list"][:k] if lst is None else lst
    return R.bound(Md, master["J"][np.ix_(lst, lst)])


@pytest.fixture(scope="module")
def forward(master):
    out = {}
    for name, (mp, cnts) in BATCHES.items():
        Mh = _pack([master["A"] * R.LD(SCALES[n]) for n in range(len(cnts))], master["ldj"])
        lists = [(master["list"][:k], np.ones(k)) for k in cnts]
        out[name] = dict(Mh=Mh, lists=lists, res=_apply(Mh, lists, mp))
    return out


@pytest.mark.parametrize("name,k", [(nm, k) for nm, (_, cs) in BATCHES.items() for k in cs])
def test_forward_list_against_reference(master, forward, name, k):
    n = BATCHES[name][1].index(k)
    f = forward[name]
    got = f["res"]["M"][n]
    assert f["res"]["status"][n] == 0 and _padding_untouched(got)
    assert f["res"]["batch_k"][n] == (k + 15) // 16 * 16
    # the pivot-block inverse the call leaves in G: M_DD^-1 in the k x k corner and exactly zero around it -- the frame of the blocked inverse
    # holds the identity there, and the panel products run over the padded K.  (A neuron without pivots never reaches the LDS inversion
    # of pgl_flip_apply, which is what writes G on that path.)
    G = f["res"]["G"][n]
    if k > 0 or BATCHES[name][0] is not None:
        assert not G[k:, :].any() and not G[:, k:].any(), "G is not zero outside its %d x %d corner" % (k, k)
    if k == 0:
        assert np.array_equal(_bits(got), _bits(f["Mh"][n])), "d_cnt = 0 must leave the tableau alone, bit for bit"
        return
    S = master["list"][:k]
    ref = R.scale_swept(master["swept"][k], S, SCALES[n])
    err, eg, bnd = _lower_err(got, ref), R.relerr(G[:k, :k], -ref[np.ix_(S, S)]), _bound(master, k)
    print("TABLEAU %s d_cnt=%d  err %.2e  G %.2e  bound %.2e" % (name, k, err, eg, bnd))
    assert err <= bnd and eg <= bnd


@pytest.mark.parametrize("name,k", [("apply", 127), ("chunk256", 129), ("chunk512", 385), ("chunk512", 3)])
def test_a_neuron_alone_equals_its_result_in_the_batch(forward, name, k):
    n = BATCHES[name][1].index(k)
    f = forward[name]
    alone = _apply(f["Mh"][n:n + 1], f["lists"][n:n + 1], BATCHES[name][0])
    assert alone["status"][0] == 0
    assert np.array_equal(_bits(alone["M"][0]), _bits(f["res"]["M"][n]))


def test_two_chunks_in_a_row_equal_one_sweep_of_the_whole_set(master):
    """a 441-row list as 256 + 185 (the initial sweep of tests/test_gpu_parity.py::test_sweep_vs_oracle_large_initial_active_set), beside a
    300-row list (256 + 44) and a 100-row one (100 + 0), and then the definition itself on the result:
    M_SS = -J_SS^-1, M_Sh = J_SS^-1 h_S, the Schur complement on the rest.
    Bound: each call is held to 8 Md 2^-53 kappa_2 of its own pivot block -- J_S1S1 and the Schur complement of it in J_SS, whose condition
    numbers are both at most kappa_2(J_SS) (eigenvalue interlacing) -- so the pair to twice the bound of the whole set."""
    cnts = [441, 300, 100]
    Mh = _pack([master["A"] * R.LD(SCALES[n]) for n in range(3)], master["ldj"])
    first = [(master["list"][:min(k, 256)], np.ones(min(k, 256))) for k in cnts]
    second = [(master["list"][256:k], np.ones(max(k - 256, 0))) for k in cnts]
    res = _apply(Mh, [first, second], [256, 185], calls=2)
    assert res[1]["batch_k"].tolist() == [192, 48, 0]
    for n, k in enumerate(cnts):
        S = master["list"][:k]
        got = res[1]["M"][n]
        assert res[1]["status"][n] == 0 and _padding_untouched(got)
        err, bnd = _lower_err(got, R.scale_swept(master["swept"][k], S, SCALES[n])), 2 * _bound(master, k)
        print("TABLEAU two chunks rows=%d  err %.2e  bound %.2e" % (k, err, bnd))
        assert err <= bnd
    assert np.array_equal(_bits(res[1]["M"][2]), _bits(res[0]["M"][2])), "the neuron with nothing left in the second chunk was touched"
    # the definition, on the 441-row neuron (c = 1)
    J, h, S = R.ld(master["J"]), R.ld(master["h"]), master["list"][:441]
    rest = np.setdiff1d(np.arange(D + 1), S)
    P = R.inv_spd(master["J"][np.ix_(S, S)])
    low = np.tril(res[1]["M"][0][:Md, :Md])
    got = low + np.tril(low, -1).T
    bnd = 2 * _bound(master, 441)
    JRS = J[np.ix_(rest, S)]
    for what, g, want in (("M_SS", got[np.ix_(S, S)], -P), ("M_Sh", got[S, D + 1], P @ h[S]),
                          ("Schur", got[np.ix_(rest, rest)], J[np.ix_(rest, rest)] - JRS @ P @ JRS.T), ("r", got[rest, D + 1], h[rest] - JRS @ P @ h[S])):
        err = R.relerr(g, want)
        print("TABLEAU definition %s  err %.2e  bound %.2e" % (what, err, bnd))
        assert err <= bnd


def test_reverse_and_mixed_lists(master):
    """after a forward sweep on S (bias + 24 blocks, 97 rows): neuron 0 reverses 9 of the blocks and forwards 12 new ones in one call (84
    rows; the result is the sweep of A on the net set), neuron 1 has nothing to do (kept bit for bit), neuron 2 reverses all of S (A comes
    back).  Bound: the sum of the two calls' bounds, each from its own pivot block as it stood before the call."""
    rng = np.random.default_rng(7)
    A, J = master["A"], master["J"]
    allb = rng.permutation(N)
    on, new = np.sort(allb[:24]), np.sort(allb[24:36])
    rev = np.sort(rng.choice(on, 9, replace=False))
    S = np.array([D] + _rows(on))
    M1 = R.sweep(A, S, np.ones(len(S)))
    mixed = np.array(_rows(np.sort(np.concatenate([rev, new]))))
    sg = np.array([-1.0 if r // B in set(rev.tolist()) else 1.0 for r in mixed])
    net = np.array([D] + _rows(np.sort(np.concatenate([np.setdiff1d(on, rev), new]))))
    Mnet = R.sweep(A, net, np.ones(len(net)))
    sc = [1.0, 4.0, 0.5]
    Mh = _pack([A * R.LD(c) for c in sc], master["ldj"])
    first = [(S, np.ones(len(S)))] * 3
    second = [(mixed, sg), (np.zeros(0, dtype=int), np.zeros(0)), (S, -np.ones(len(S)))]
    res = _apply(Mh, [first, second], None, calls=2)
    assert res[1]["status"].tolist() == [0, 0, 0] and res[1]["batch_k"].tolist() == [96, 0, 112]
    b1 = R.bound(Md, J[np.ix_(S, S)])
    for n in range(3):
        e = _lower_err(res[0]["M"][n], R.scale_swept(M1, S, sc[n]))
        print("TABLEAU forward S neuron %d  err %.2e  bound %.2e" % (n, e, b1))
        assert e <= b1 and _padding_untouched(res[1]["M"][n])
    b2 = R.bound(Md, np.asarray(M1[np.ix_(mixed, mixed)], dtype=np.float64))
    e = _lower_err(res[1]["M"][0], Mnet)
    print("TABLEAU mixed list  err %.2e  bound %.2e (%.2e + %.2e)" % (e, b1 + b2, b1, b2))
    assert e <= b1 + b2
    assert np.array_equal(_bits(res[1]["M"][1]), _bits(res[0]["M"][1]))
    e = _lower_err(res[1]["M"][2], A * R.LD(sc[2]))
    print("TABLEAU forward then reverse  err %.2e  bound %.2e" % (e, 2 * b1))
    assert e <= 2 * b1


@pytest.mark.parametrize("name,k", [("apply", 125), ("chunk256", 253)])
def test_block_rows_that_do_not_ascend(master, name, k):
    """the same set with its blocks in a shuffled order (bias still first): the same tableau as the ascending list's, to the same reference.
    A 64-pivot tile of the gather and the fix-up then holds rows from both ends of the tableau (s_min, s_piv)."""
    rng = np.random.default_rng(k)
    asc = master["list"][:k]
    blocks = asc[1:].reshape(-1, B)
    shuf = np.concatenate([[D], blocks[rng.permutation(len(blocks))].ravel()])
    assert sorted(shuf.tolist()) == sorted(asc.tolist()) and not np.all(np.diff(shuf[1:]) > 0)
    sc = [2.0, 0.5]
    Mh = _pack([master["A"] * R.LD(c) for c in sc], master["ldj"])
    res = _apply(Mh, [(asc, np.ones(k)), (shuf, np.ones(k))], BATCHES[name][0])
    bnd = _bound(master, k)
    for n in range(2):
        err = _lower_err(res["M"][n], R.scale_swept(master["swept"][k], asc, sc[n]))
        print("TABLEAU %s %s blocks rows=%d  err %.2e  bound %.2e" % (name, ("ascending", "shuffled")[n], k, err, bnd))
        assert res["status"][n] == 0 and err <= bnd and _padding_untouched(res["M"][n])


@pytest.mark.parametrize("name,k", [("apply", 17), ("chunk256", 129)])
def test_a_singular_pivot_is_flagged_on_its_neuron_only(master, forward, name, k):
    """a zeroed pivot block: status bit 2 on that neuron, every other neuron's tableau the same bits as without it"""
    f = forward[name]
    bad = BATCHES[name][1].index(k)
    Mh = f["Mh"].copy()
    lst = master["list"][:k]
    for i in lst:
        for j in lst:
            if i >= j:
                Mh[bad, i, j] = 0.0
    res = _apply(Mh, f["lists"], BATCHES[name][0])
    assert res["status"][bad] & 2
    for n in range(len(f["lists"])):
        if n != bad:
            assert res["status"][n] == 0 and np.array_equal(_bits(res["M"][n]), _bits(f["res"]["M"][n]))


# ---------------------------------------------------------------------------------------------------------------- pgl_flip_visit_order
@pytest.mark.parametrize("Bv", [1, 3, 5, 8, 11, 32])
def test_visit_order_is_a_pure_permutation(Bv):
    """M = P J P' exactly (np.ix_), for the compiled block sizes and the run-time-B instantiation; N = 37 (no tile size divides N B), a
    source with its own leading dimension, NaN above the source's diagonal; the bias and potential rows are gathered by position.
    The kernel writes whole diagonal blocks (mirrored) and nothing else above the diagonal."""
    import torch
    from pyglm_amd._lib import FlipState, call
    Nv, nb = 37, 3
    Dv = Nv * Bv
    rng = np.random.default_rng(Bv)
    v = ctypes.c_int()
    call("pgl_sweep_dims", Nv, Bv, 1, None, None, ctypes.byref(v))
    ldj, lds = v.value, v.value + 10
    low = np.tril(rng.standard_normal((nb, Dv + 2, Dv + 2)))
    sym = low + np.transpose(np.tril(low, -1), (0, 2, 1))
    src = np.full((nb, lds, lds), np.nan)
    il = np.tril_indices(Dv + 2)
    for n in range(nb):
        src[n][il] = low[n][il]
    perm = np.stack([rng.permutation(Nv) for _ in range(nb)]).astype(np.int32)
    dev = torch.device("cuda:0")
    Jd, Mt, pd = torch.from_numpy(src).to(dev), torch.full((nb, ldj, ldj), SENT, dtype=torch.float64, device=dev), torch.from_numpy(perm).to(dev)
    s = FlipState(M=Mt.data_ptr(), ldj=ldj, strideM=ldj * ldj, nb=nb, N=Nv, B=Bv, perm=pd.data_ptr(), visit_order=1)
    call("pgl_flip_visit_order", ctypes.byref(s), ctypes.c_void_p(Jd.data_ptr()), lds, lds * lds, None)
    torch.cuda.synchronize()
    got = Mt.cpu().numpy()
    r = np.arange(Dv + 2)
    blk = np.where(r < Dv, r // Bv, -1 - r)                                    # the bias and potential rows are blocks of their own
    written = (r[:, None] >= r[None, :]) | (blk[:, None] == blk[None, :])
    for n in range(nb):
        srow = np.concatenate([(perm[n][:, None] * Bv + np.arange(Bv)[None, :]).ravel(), [Dv, Dv + 1]])
        want = np.full((ldj, ldj), SENT)
        want[:Dv + 2, :Dv + 2] = np.where(written, sym[n][np.ix_(srow, srow)], SENT)
        assert np.array_equal(_bits(got[n]), _bits(want)), "B = %d neuron %d" % (Bv, n)
