"""The cases and references of tests/test_gpu_contraction.py checked without a GPU (tests/_contraction_cases.py): the dyadic references do
not depend on the summation order (int64 cross-check, magnitudes below 2^52), the nz derivations select the intended Gram kernel under the
dispatch rule restated there, every variant of the dispatch table has a case, and check_output catches what it is there to catch."""
import pytest
import torch

from tests import _contraction_cases as C


def _gram_int_check(c, z, accumulate):
    ref, bound = C.gram_ref(c, accumulate)
    assert bound is None
    Xd = c["X"][:c["Tp"], :c["D"]]
    return C.scaled_int_check(Xd, Xd, c["W"][:c["Tp"], z], c["J0"][z], 1.0, 1.0 if accumulate else 0.0, ref[z])


@pytest.mark.parametrize("family,D,nz,Tp", [("wave8", 130, C.nz_wave8(130, 64), 80), ("wave8", 256, 5, 48), ("fine", 129, 3, 64), ("fine", 384, 2, 32),
                                            ("fine several items", 130, C.nz_fine_second_item(64), 48)])
def test_dyadic_gram_reference_is_order_independent(family, D, nz, Tp):
    c = C.gram_case("exact", D, nz, Tp)
    for z in (0, nz - 1):
        for accumulate in (0, 1):
            assert _gram_int_check(c, z, accumulate) < 2 ** 30
    # the inputs are what the module says: a quarter zeros, weights in [0, 4], poison from the even column count / from nz on
    Xd = c["X"][:Tp, :D]
    assert 0.15 < float((Xd == 0).double().mean()) < 0.40 and float(Xd.abs().max()) <= 4.0
    assert float(c["W"][:Tp, :nz].min()) >= 0.0 and float(c["W"][:Tp, :nz].max()) <= 4.0
    assert bool(torch.isnan(c["X"][:, c["x_cols"] & ~1:]).all()) and bool(torch.isnan(c["W"][:, nz:]).all())
    assert c["X"].shape[0] == c["W"].shape[0] == Tp + 16 and bool(torch.isnan(c["X"][Tp:]).all()) and bool(torch.isnan(c["W"][Tp:]).all())
    assert (c["x_cols"] & ~1) >= D and c["x_cols"] <= c["ldx"] and c["ldx"] % 2 == 0 and c["ldw"] > nz and c["ldj"] > D
    assert not bool(torch.isnan(c["X"][:Tp, :c["x_cols"] & ~1]).any())


def _one_of_each_family():
    cases = C.batched_cases() + C.skinny_cases()
    seen, out = set(), []
    for c in cases:                                   # per family: the first case that reads C and has per-batch K, else the first
        key = c["family"]
        if key not in seen and c["beta"] != 0.0 and c["batch_k"]:
            seen.add(key)
            out.append(c)
    assert seen == {c["family"] for c in cases}
    return out


@pytest.mark.parametrize("case", _one_of_each_family(), ids=lambda c: c["id"])
def test_dyadic_contraction_reference_is_order_independent(case):
    c = C.contraction_case("exact", case["M"], case["N"], case["K"], C.NBATCH, case["alpha"], case["beta"], tri=case["tri"],
                           batch_k=case["batch_k"], shared=case["shared"])
    assert c["bound"] is None
    for b in range(C.NBATCH):
        kb, s = case["batch_k"][b], 0 if case["shared"] else b
        if kb == 0:
            assert not bool(c["written"][b].any())
            continue
        big = C.scaled_int_check(c["A"][s, :kb, :case["M"]], c["B"][s, :kb, :case["N"]], None, c["C0"][b], case["alpha"], case["beta"], c["ref"][b])
        assert big < 2 ** 30
    Me, Ne = c["a_cols"] & ~1, c["b_cols"] & ~1
    assert Me >= case["M"] and Ne >= case["N"] and c["lda"] % 2 == 0 and c["ldb"] % 2 == 0 and c["a_cols"] <= c["lda"] and c["b_cols"] <= c["ldb"]
    assert bool(torch.isnan(c["A"][:, :, Me:]).all()) and bool(torch.isnan(c["B"][:, :, Ne:]).all())
    if not case["shared"]:
        assert bool(torch.isnan(c["A"][1, 16:]).all()) and bool(torch.isnan(c["B"][2]).all())
    assert not bool(torch.isnan(c["A"][0, :, :Me]).any())


def test_dyadic_single_contractions_are_order_independent():
    T, nloc, Dk = 77, 130, 48
    c = C.contraction_case("exact", T, nloc, Dk, 1, 1.0, 0.0, full_cols=True)
    assert C.scaled_int_check(c["A"][0, :, :T], c["B"][0, :, :nloc], None, c["C0"][0], 1.0, 0.0, c["ref"][0]) < 2 ** 30
    assert c["a_cols"] == c["lda"] > T and c["b_cols"] == c["ldb"] > nloc and not bool(torch.isnan(c["A"]).any() | torch.isnan(c["B"]).any())
    M, N, beta = 66, 129, 1.0
    c = C.contraction_case("exact", M, N, 96, 1, 1.0, beta)
    assert C.scaled_int_check(c["A"][0, :, :M], c["B"][0, :, :N], None, c["C0"][0], 1.0, beta, c["ref"][0]) < 2 ** 30


def test_alpha_beta_and_k_stay_inside_the_exact_premise():
    assert {x for ab in C.ALPHA_BETA for x in ab} <= {1.0, -1.0, 2.0, -0.5, 0.0} and max(C.KS) <= 96 and all(K % 16 == 0 for K in C.KS)
    assert C.ALPHA_BETA[:4] == [(1.0, 0.0), (-0.5, 0.0), (1.0, 1.0), (-1.0, 1.0)] and C.ALPHA_BETA[4:] == [(2.0, 1.0), (1.0, -0.5)]


@pytest.mark.parametrize("cu", C.CU_COUNTS)
def test_nz_derivations_select_the_intended_gram_kernel(cu):
    for D, _ in C.GRAM_WAVE8:
        nz, tiles = C.nz_wave8(D, cu), C.gram_tiles(D)
        assert tiles == 3 and nz % 2 == 1
        assert tiles * ((nz + 1) // 2) >= 2 * cu and C.gram_kernel(D, nz, cu) == "gram_wave8"
        assert nz == 1 or (tiles * ((nz - 2 + 1) // 2) < 2 * cu and C.gram_kernel(D, nz - 2, cu) == "gram_fine")          # the smallest odd one
        assert tiles * ((nz + 1) // 2) > cu                          # more items than CUs: every workgroup of the one-per-CU launch takes several
        assert C.gram_kernel(D, 4, cu) == "gram_fine"               # the launch its first four neurons are compared with
    assert C.nz_wave8(130, 256) == 341                               # (3 * 171 = 513 >= 512)
    for D, nz in C.GRAM_FINE:
        assert C.gram_kernel(D, nz, cu) == "gram_fine" and C.gram_fine_items_per_workgroup(D, nz, cu) == (1, 1)
    nz = C.nz_fine_second_item(cu)
    assert nz % 2 == 0 and C.gram_tiles(130) == 3 and 3 * nz // 2 < 2 * cu < 3 * nz
    assert C.gram_kernel(130, nz, cu) == "gram_fine" and C.gram_fine_items_per_workgroup(130, nz, cu) == (1, 2)
    assert C.nz_fine_second_item(256) == 300


def test_every_variant_of_the_dispatch_table_has_a_case():
    cases = C.batched_cases() + C.skinny_cases()
    got = {c["variant"] for c in cases} | {"gram_fine", "gram_wave8"}
    got |= {C.tile_variant(T, nloc, 0, 1.0, 0.0) for T, nloc, _ in C.ACTIVATION} | {C.tile_variant(M, N, 0, 1.0, b) for M, N, b in C.BORDER}
    assert got == set(C.VARIANTS)
    # the families run the variant they are named after, and the skinny family straddles the split
    for c in cases:
        if c["family"].startswith("plain"):
            assert c["variant"].startswith(c["family"])
        if c["family"] in ("tri1", "tri2"):
            assert c["variant"].startswith("tri<2,2,1>") and c["kernel"] == 0
    assert {(c["M"], c["variant"]) for c in C.skinny_cases()} == {(129, "skinny+tiles"), (144, "skinny+tiles"), (145, "tri<2,2,1> cinit"),
                                                                  (258, "skinny+tiles")}
    # every (family, K), every (family, alpha / beta), and batch_k both ways in every family
    for family in {c["family"] for c in cases}:
        mine = [c for c in cases if c["family"] == family]
        assert {c["K"] for c in mine} == set(C.KS) and {bool(c["batch_k"]) for c in mine} == {False, True}
        if family != "skinny":
            assert {(c["alpha"], c["beta"]) for c in mine} == set(C.ALPHA_BETA)
    assert len({c["id"] for c in cases}) == len(cases)
    assert {C.tile_variant(T, nloc, 0, 1.0, 0.0) for T, nloc, _ in C.ACTIVATION} == {"plain<2,2,1>", "plain<1,4,1>", "plain<2,4,1>"}


def test_written_sets():
    m1, m2 = C.tile_mask(200, 200, 1), C.tile_mask(200, 200, 2)
    assert bool(m1[128, 0]) and bool(m1[0, 127]) and not bool(m1[127, 128]) and bool(m1[199, 199]) and bool((m2 == m1.T).all())
    assert bool(C.tile_mask(65, 129, 0).all())


def test_check_output_catches_a_stray_write_a_wrong_element_and_a_poison_read():
    c = C.contraction_case("exact", 129, 129, 32, C.NBATCH, 1.0, 1.0, tri=1, batch_k=[32, 16, 0])
    before = C.poisoned_buffer(c["C0"], c["written"], C.NBATCH + 1, c["rows"], c["ldc"])
    good = before.clone()
    good[:C.NBATCH, :129, :129] = torch.where(c["written"], c["ref"], before[:C.NBATCH, :129, :129])
    C.check_output(good, before, c["ref"], None, c["written"])
    for where_, value in (((0, 129, 0), 0.0), ((0, 0, 129), 0.0), ((0, 0, 128), 1.0), ((2, 5, 5), 1.0), ((3, 0, 0), 0.0), ((1, 7, 7), NAN_),
                          ((0, 128, 128), None)):
        bad = good.clone()
        bad[where_] = bad[where_] + 0.125 if value is None else value
        with pytest.raises(AssertionError):
            C.check_output(bad, before, c["ref"], None, c["written"])
    r = C.contraction_case("real", 17, 300, 96, C.NBATCH, -0.5, 0.0)
    before = C.poisoned_buffer(r["C0"], r["written"] & False, C.NBATCH + 1, r["rows"], r["ldc"])
    assert bool(torch.isnan(before).all())
    good = before.clone()
    good[:C.NBATCH, :17, :300] = r["ref"]
    C.check_output(good, before, r["ref"], r["bound"], r["written"])
    # the bound is a few hundred ulp of the magnitudes, not a tolerance that forgives a wrong k-step
    assert float((r["bound"] / r["ref"].abs().clamp_min(1e-3)).median()) < 1e-12
    bad = good.clone()
    bad[1, 3, 3] += 1e-9
    with pytest.raises(AssertionError):
        C.check_output(bad, before, r["ref"], r["bound"], r["written"])


NAN_ = float("nan")
