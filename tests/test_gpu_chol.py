"""The weight draw on its own: pgl_active_index + pgl_sample_weights (pgl_chol.hip) through CholState, against the longdouble reference of
tests/_dense_ref.py (checked on the CPU by tests/test_dense_ref_host.py).

What the kernels do (pgl_chol.hip): compact the active block, blocked upper Cholesky on 64-wide panels grouped into super-panels of 6 (8 when
ldact > 8192), the forward solve riding along as column na, the backward solve panel by panel.  The sizes below sit on every edge the code
names: a short last block against na % 64 == 0 (the h column solved inside potrf_diag_kernel or by a panel solve), the super-panel edge
(384 / 385 at SP = 6, 512 / 513 at SP = 8), neurons of very different na in one batch (dim_mode 0, 1, 3 of the contraction), the na_max hint.

Tolerance: max |x_dev - x_ref| / max |x_ref| <= 8 n 2^-53 kappa_2(J_aa) with n = na, for the draw x, for mu (the run with z = 0) and for
x - mu = U^-1 z (which pins the factor itself: a quadratic form is blind to a rotation of the draw).  Everything else is exact.
Each case prints its measured maxima next to the bound."""
import ctypes

import numpy as np
import pytest

from tests import _dense_ref as R

pytestmark = pytest.mark.gpu

SENT = -777.25
N1, B1 = 800, 1
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 383, 384, 385, 448, 449, 641, 768, 769]      # one neuron each, B = 1: na = sum(a) + 1
SIZES_SP8 = SIZES + [512, 513]                                                         # the super-panel edge of SP = 8
ENDS_ON = (129, 385, 449)                                                              # scattered sets with the first and the last block forced on


def _ldj(N, B):
    from pyglm_amd._lib import call
    v = ctypes.c_int()
    call("pgl_sweep_dims", N, B, 1, None, None, ctypes.byref(v))
    return v.value


def _pack(systems, N, B, ldj):
    """[(J, h)] of size D + 1 (bias last) -> (nb, ldj, ldj) in the sweep's layout: lower triangle, bias row D, potential row D + 1.  Everything
    that is not the valid lower triangle -- the strict upper triangle, the padding -- is NaN: the contract says "lower triangle valid"."""
    D = N * B
    out = np.full((len(systems), ldj, ldj), np.nan)
    il = np.tril_indices(D + 1)
    for n, (J, h) in enumerate(systems):
        out[n][il] = J[il]
        out[n, D + 1, :D + 1] = h
        out[n, D + 1, D + 1] = 0.0
    return out


def _act(a_row, B, D):
    return np.concatenate([(np.nonzero(a_row)[0][:, None] * B + np.arange(B)[None, :]).ravel(), [D]]).astype(np.int64)


def _run(Jd, a, z, N, B, na_max=None, ldact=None, ldc=None, ldz=None):
    """pgl_active_index + pgl_sample_weights on guarded buffers: Ac, hc, Tinv NaN, W and b a sentinel, act / na -1.  z: (nb, D + 1) host."""
    import torch
    from pyglm_amd._lib import CholState, call
    dev = Jd.device
    nb, ldj, D = Jd.shape[0], Jd.shape[1], N * B
    ldact, ldc, ldz = ldact or D + 1, ldc or ldj, ldz or D + 1
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    a_d = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    z_d = torch.from_numpy(np.ascontiguousarray(z[:, :ldz], dtype=np.float64)).to(dev)
    act, na = torch.full((nb, ldact), -1, **i32), torch.full((nb,), -1, **i32)
    Ac = torch.full((nb, ldc, ldc), float("nan"), **f64)
    hc, Tinv = torch.full((2, nb, ldc), float("nan"), **f64), torch.full((nb, 64, 64), float("nan"), **f64)
    W, b, status = torch.full((nb, D), SENT, **f64), torch.full((nb,), SENT, **f64), torch.zeros(nb, **i32)
    s = CholState(J=Jd.data_ptr(), ldj=ldj, strideJ=ldj * ldj, a=a_d.data_ptr(), act=act.data_ptr(), ldact=ldact, na=na.data_ptr(),
                  Ac=Ac.data_ptr(), ldc=ldc, strideC=ldc * ldc, hc=hc.data_ptr(), Tinv=Tinv.data_ptr(), z=z_d.data_ptr(), ldz=ldz,
                  W=W.data_ptr(), b=b.data_ptr(), nb=nb, N=N, B=B, status=status.data_ptr())
    out = {}
    try:
        call("pgl_active_index", ctypes.byref(s), None)
        torch.cuda.synchronize()
        out["act"], out["na"] = act.cpu().numpy(), na.cpu().numpy()
        call("pgl_sample_weights", ctypes.byref(s), D + 1 if na_max is None else na_max, None)
    finally:
        torch.cuda.synchronize()
        out.update(W=W.cpu().numpy(), b=b.cpu().numpy(), status=status.cpu().numpy(), Ac_untouched=bool(torch.isnan(Ac).all()))
    return out


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _z(rng, a, B, D):
    """standard normals, NaN beyond each neuron's na (only the first na[n] are consumed)"""
    z = rng.standard_normal((a.shape[0], D + 1))
    for n in range(a.shape[0]):
        z[n, int(a[n].sum()) * B + 1:] = np.nan
    return z


def _z0(z):
    return np.where(np.isnan(z), np.nan, 0.0)


def _check_neuron(tag, out, out0, n, a_row, B, D, ref):
    """exact: act, na, zeros, status.  To the bound: x, mu, x - mu."""
    act = _act(a_row, B, D)
    na = len(act)
    assert out["na"][n] == na and out0["na"][n] == na
    assert np.array_equal(out["act"][n, :na], act)
    assert np.all(out["act"][n, na:] == -1), "act written beyond na"
    assert out["status"][n] == 0 and out0["status"][n] == 0
    off = np.repeat(np.asarray(a_row) == 0, B)
    for o in (out, out0):
        assert np.array_equal(_bits(o["W"][n][off]), _bits(np.zeros(int(off.sum())))), "W is not exactly +0 where a = 0"
    x = np.concatenate([out["W"][n][act[:-1]], [out["b"][n]]])
    mu = np.concatenate([out0["W"][n][act[:-1]], [out0["b"][n]]])
    mu_ref, dx_ref, bnd = ref
    ex, em, ed = R.relerr(x, mu_ref + dx_ref), R.relerr(mu, mu_ref), R.relerr(x - mu, dx_ref)
    print("CHOL %s na=%d  x %.2e  mu %.2e  x-mu %.2e  bound %.2e" % (tag, na, ex, em, ed, bnd))
    assert ex <= bnd and em <= bnd and ed <= bnd, (ex, em, ed, bnd)


# ---------------------------------------------------------------------------------------------------------------- the B = 1 batch
@pytest.fixture(scope="module")
def big():
    """18 neurons of N = 800, B = 1 on one posterior J (801 rows with the bias; kappa_2 about 3.6): scattered active sets up to na = 449,
    nested prefixes above -- the factor of a leading block is the leading block of the factor, so ONE longdouble factorisation serves
    641 ... 769 and the SP = 8 edge 512 / 513."""
    import torch
    rng = np.random.default_rng(20240)
    D = N1 * B1
    J, h = R.wellcond_system(D + 1, rng)
    a = np.zeros((len(SIZES_SP8), N1), dtype=np.int32)
    for n, na in enumerate(SIZES_SP8):
        if na > 449:
            a[n, :na - 1] = 1
        elif na in ENDS_ON:
            a[n, [0, N1 - 1]] = 1
            a[n, 1 + rng.choice(N1 - 2, na - 3, replace=False)] = 1
        else:
            a[n, rng.choice(N1, na - 1, replace=False)] = 1
    z = _z(rng, a, B1, D)
    U_full = R.chol_upper(J[:D, :D])
    w_full = R.solve_upper_t(U_full, J[:D, D])
    refs = []
    for n, na in enumerate(SIZES_SP8):
        act = _act(a[n], B1, D)
        Jaa = J[np.ix_(act, act)]
        U = R.bordered_prefix_factor(U_full, w_full, J[D, D], na - 1) if na > 449 else R.chol_upper(Jaa)
        mu, dx = R.draw_from_factor(U, h[act], z[n, :na])
        refs.append((mu, dx, R.bound(na, Jaa)))
    ldj = _ldj(N1, B1)
    Jh = _pack([(J, h)], N1, B1, ldj)
    Jd = torch.from_numpy(Jh).to("cuda:0").repeat(len(SIZES_SP8), 1, 1).contiguous()
    return dict(J=J, h=h, a=a, z=z, refs=refs, Jd=Jd, D=D)


@pytest.fixture(scope="module")
def big_sp6(big):
    """the 16 listed sizes with production's hint na_max = D + 1: the draw and the run with z = 0"""
    k = len(SIZES)
    return (_run(big["Jd"][:k], big["a"][:k], big["z"][:k], N1, B1), _run(big["Jd"][:k], big["a"][:k], _z0(big["z"][:k]), N1, B1))


@pytest.fixture(scope="module")
def big_sp8(big):
    """all 18 with ldact = 8200: the act buffer is nb x 8200 ints and the factorisation takes super-panels of 8"""
    return (_run(big["Jd"], big["a"], big["z"], N1, B1, ldact=8200), _run(big["Jd"], big["a"], _z0(big["z"]), N1, B1, ldact=8200))


@pytest.mark.parametrize("na", SIZES)
def test_draw_against_reference(big, big_sp6, na):
    n = SIZES.index(na)
    _check_neuron("sp6", big_sp6[0], big_sp6[1], n, big["a"][n], B1, big["D"], big["refs"][n])


def test_bias_only_neuron_is_the_scalar_law(big, big_sp6):
    """a all zero: b = h_D / J_DD + z / sqrt(J_DD)"""
    D = big["D"]
    want = big["h"][D] / big["J"][D, D] + big["z"][0, 0] / np.sqrt(big["J"][D, D])
    assert abs(big_sp6[0]["b"][0] - want) <= 8 * R.U53 * abs(want)
    assert not big_sp6[0]["W"][0].any()


@pytest.mark.parametrize("na", SIZES_SP8)
def test_draw_against_reference_with_super_panels_of_8(big, big_sp8, na):
    """(checked against the reference, not bit for bit against SP = 6: the rank of the trailing updates differs)"""
    n = SIZES_SP8.index(na)
    _check_neuron("sp8", big_sp8[0], big_sp8[1], n, big["a"][n], B1, big["D"], big["refs"][n])


@pytest.mark.parametrize("k", [len(SIZES), SIZES.index(449) + 1])
def test_the_hint_does_not_move_a_bit(big, big_sp6, k):
    """na_max = max(na) against na_max = D + 1 (what production passes): 'a hint must not move a bit of the result'.  With all 16 neurons
    the tight hint is 769; with the first 13 it is 449, and the row-panel solve at column 384 then sees a remainder of 66 columns instead
    of 418 -- another tile shape of the contraction, which promises the same bits."""
    tight = _run(big["Jd"][:k], big["a"][:k], big["z"][:k], N1, B1, na_max=max(SIZES[:k]))
    assert np.array_equal(tight["status"], big_sp6[0]["status"][:k])
    for n, na in enumerate(SIZES[:k]):
        assert np.array_equal(_bits(tight["W"][n]), _bits(big_sp6[0]["W"][n])) and _bits(tight["b"][n]) == _bits(big_sp6[0]["b"][n]), \
            "na_max = %d moved the draw of the neuron with na = %d" % (max(SIZES[:k]), na)


@pytest.mark.parametrize("na", [65, 385, 769])
def test_a_neuron_alone_equals_its_result_in_the_batch(big, big_sp6, na):
    n = SIZES.index(na)
    alone = _run(big["Jd"][n:n + 1], big["a"][n:n + 1], big["z"][n:n + 1], N1, B1)
    assert alone["status"][0] == 0
    assert np.array_equal(_bits(alone["W"][0]), _bits(big_sp6[0]["W"][n])) and _bits(alone["b"][0]) == _bits(big_sp6[0]["b"][n])


def test_an_indefinite_block_is_flagged_and_spares_the_other_neurons(big, big_sp6):
    """one diagonal entry of one neuron's active block with its sign flipped: the call returns, that neuron carries status bit 4, every other
    neuron's draw is the same bits as without it (the handled error path the engine turns into LinAlgError)"""
    k, bad = len(SIZES), SIZES.index(129)
    Jd = big["Jd"][:k].clone()
    r = int(_act(big["a"][bad], B1, big["D"])[70])
    Jd[bad, r, r] = -Jd[bad, r, r]
    out = _run(Jd, big["a"][:k], big["z"][:k], N1, B1)
    assert out["status"][bad] & 4
    for n in range(k):
        if n != bad:
            assert out["status"][n] == 0
            assert np.array_equal(_bits(out["W"][n]), _bits(big_sp6[0]["W"][n])) and _bits(out["b"][n]) == _bits(big_sp6[0]["b"][n])


# ---------------------------------------------------------------------------------------------------------------- B = 5: gathers in runs of B
B5_NAMES = ["sparse", "half", "dense", "all_on", "all_off"]


@pytest.fixture(scope="module")
def b5():
    import torch
    rng = np.random.default_rng(77)
    N, B = 90, 5
    D = N * B
    a = np.zeros((5, N), dtype=np.int32)
    for n, p in enumerate((0.1, 0.5, 0.9)):
        a[n] = rng.random(N) < p
    a[3] = 1                                                    # na = 451
    systems = [R.wellcond_system(D + 1, rng) for _ in range(5)]
    z = _z(rng, a, B, D)
    refs = []
    for n in range(5):
        act = _act(a[n], B, D)
        J, h = systems[n]
        Jaa = J[np.ix_(act, act)]
        mu, dx = R.draw_from_factor(R.chol_upper(Jaa), h[act], z[n, :len(act)])
        refs.append((mu, dx, R.bound(len(act), Jaa)))
    Jd = torch.from_numpy(_pack(systems, N, B, _ldj(N, B))).to("cuda:0")
    return dict(a=a, refs=refs, N=N, B=B, D=D, runs=(_run(Jd, a, z, N, B), _run(Jd, a, _z0(z), N, B)))


@pytest.mark.parametrize("which", B5_NAMES)
def test_blocks_of_five_against_reference(b5, which):
    n = B5_NAMES.index(which)
    assert int(b5["a"][3].sum()) * b5["B"] + 1 == 451 and not b5["a"][4].any()
    _check_neuron("B5 " + which, b5["runs"][0], b5["runs"][1], n, b5["a"][n], b5["B"], b5["D"], b5["refs"][n])


# ---------------------------------------------------------------------------------------------------------------- kappa_2 = 1e6
KAPPA_SIZES = [129, 385]


@pytest.fixture(scope="module")
def illcond():
    """active blocks with a prescribed spectrum (Q diag(lam) Q', lam log-spaced to kappa_2 = 1e6), so that the bound is exercised where it is
    not tiny: about 1e-7"""
    import torch
    rng = np.random.default_rng(99)
    D = N1 * B1
    a = np.zeros((2, N1), dtype=np.int32)
    systems, refs = [], []
    for n, na in enumerate(KAPPA_SIZES):
        a[n, rng.choice(N1, na - 1, replace=False)] = 1
    z = _z(rng, a, B1, D)
    for n, na in enumerate(KAPPA_SIZES):
        act = _act(a[n], B1, D)
        J, h = np.eye(D + 1), rng.standard_normal(D + 1)
        Jaa, _ = R.spectrum_system(na, 1e6, rng)
        J[np.ix_(act, act)] = Jaa
        systems.append((J, h))
        mu, dx = R.draw_from_factor(R.chol_upper(Jaa), h[act], z[n, :na])
        refs.append((mu, dx, R.bound(na, Jaa)))
    Jd = torch.from_numpy(_pack(systems, N1, B1, _ldj(N1, B1))).to("cuda:0")
    return dict(a=a, refs=refs, D=D, runs=(_run(Jd, a, z, N1, B1), _run(Jd, a, _z0(z), N1, B1)))


@pytest.mark.parametrize("na", KAPPA_SIZES)
def test_ill_conditioned_block_against_reference(illcond, na):
    n = KAPPA_SIZES.index(na)
    assert 5e-8 < illcond["refs"][n][2] < 5e-7
    _check_neuron("kappa 1e6", illcond["runs"][0], illcond["runs"][1], n, illcond["a"][n], B1, illcond["D"], illcond["refs"][n])


# ---------------------------------------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("what", ["na_max_zero", "odd_ldc", "short_ldz"])
def test_refused_arguments_raise_and_launch_nothing(what):
    """na_max = 0, an odd ldc, ldz < na_max: PglError, and W and b keep their sentinel, the scratch its NaN, status its zero"""
    import torch
    from pyglm_amd._lib import CholState, PglError, call
    rng = np.random.default_rng(2)
    N, B = 12, 2
    D = N * B
    ldj = _ldj(N, B)
    dev = torch.device("cuda:0")
    Jd = torch.from_numpy(_pack([R.wellcond_system(D + 1, rng)], N, B, ldj)).to(dev)
    a = torch.ones(1, N, dtype=torch.int32, device=dev)
    act, na = torch.zeros(1, D + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    Ac = torch.full((1, ldj + 1, ldj + 1), float("nan"), dtype=torch.float64, device=dev)
    hc = torch.full((2, 1, ldj + 1), float("nan"), dtype=torch.float64, device=dev)
    Tinv = torch.full((1, 64, 64), float("nan"), dtype=torch.float64, device=dev)
    z = torch.zeros(1, D + 1, dtype=torch.float64, device=dev)
    W, b = torch.full((1, D), SENT, dtype=torch.float64, device=dev), torch.full((1,), SENT, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def state(ldc, ldz):
        return CholState(J=Jd.data_ptr(), ldj=ldj, strideJ=ldj * ldj, a=a.data_ptr(), act=act.data_ptr(), ldact=D + 1, na=na.data_ptr(),
                         Ac=Ac.data_ptr(), ldc=ldc, strideC=ldc * ldc, hc=hc.data_ptr(), Tinv=Tinv.data_ptr(), z=z.data_ptr(), ldz=ldz,
                         W=W.data_ptr(), b=b.data_ptr(), nb=1, N=N, B=B, status=status.data_ptr())
    s = state(ldj, D + 1)
    call("pgl_active_index", ctypes.byref(s), None)
    torch.cuda.synchronize()
    assert int(na[0]) == D + 1
    s, na_max = dict(na_max_zero=(state(ldj, D + 1), 0), odd_ldc=(state(ldj + 1, D + 1), D + 1), short_ldz=(state(ldj, D), D + 1))[what]
    with pytest.raises(PglError):
        call("pgl_sample_weights", ctypes.byref(s), na_max, None)
    torch.cuda.synchronize()
    assert bool((W == SENT).all()) and bool((b == SENT).all()) and bool(torch.isnan(Ac).all()) and int(status[0]) == 0
    assert bool(torch.isnan(hc).all()) and bool(torch.isnan(Tinv).all())
