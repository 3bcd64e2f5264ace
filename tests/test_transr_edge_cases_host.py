"""Host-side checks of the fixtures in tests/transr_edge_cases.py, so that tests/test_gpu_transr_edges.py tests what
it says: every exact case is exact, the `dims` cases reach all 20 instantiations of the chunk kernel, each
tie_and_sign condition occurs, each wrap case lies past the threshold it is named for, and the thresholds restated
in the module are the constants of ge_transr.hip and ge_common.h."""
import numpy as np
import pytest

from tests import transr_edge_cases as EC
from tests import transr_ref as RR


def test_mirrored_constants_are_the_sources():
    c = EC.source_constants()
    assert (c["kChunk"], c["kAdamMaxBlocks"], c["kBlock"], c["kMaxBlocks"], c["kTrMaxDim"], c["kWave"],
            c["kPlanBlock"]) == (EC.K_CHUNK, EC.K_ADAM_MAX_BLOCKS, EC.K_BLOCK, EC.K_MAX_BLOCKS, EC.K_TR_MAX_DIM,
                                 EC.K_WAVE, EC.PLAN_BLOCK) == (16, 4096, 256, 2048, 256, 64, 1024)
    assert (EC.SCORE_WRAP, EC.PREP_WRAP, EC.EMAP_WRAP, EC.ADAM_UNIT_CAP) == (8192, 524288, 524288, 1048576)
    assert 2 * EC.SCORE_WRAP < EC.SCORE_B                      # the score kernel's loop goes round more than twice
    assert max(max(d) for d in EC.DIMS) == EC.K_TR_MAX_DIM
    # 256 x 256: the chunk kernel's dynamic LDS is exactly 64 KB
    assert 2 * EC.K_CHUNK * (256 + 256) * 4 == 65536


def test_mirrored_dispatch():
    assert [EC.nc_for(n) for n in range(1, 17)] == [2, 4, 8, 8] + [16] * 4 + [32] * 8
    assert EC.chunk_sizes([1, 16, 17, 48, 33]) == [1, 16, 16, 1, 16, 16, 16, 16, 16, 1]
    assert EC.vec_for(100, 100) == 4 and EC.vec_for(100, 100, aligned=False) == 1
    assert EC.vec_for(100, 50) == EC.vec_for(7, 256) == EC.vec_for(1, 1) == 1 and EC.vec_for(4, 4) == 4
    assert [EC.sort_key_bits(n) for n in (1, 2, 3, 4, 64, 127, 128, 1024)] == [1, 2, 2, 3, 7, 7, 8, 11]


def test_integer_tables_default_is_unchanged():
    """density=None draws what integer_tables always drew (restated here); a density only zeroes entries."""
    rng = np.random.default_rng(3)
    old = {"ent": rng.integers(-2, 3, size=(40, 12)).astype(np.float64),
           "rel": rng.integers(-2, 3, size=(6, 20)).astype(np.float64),
           "rel_matrix": rng.integers(-2, 3, size=(6, 240)).astype(np.float64)}
    new, thin = RR.integer_tables(40, 6, 12, 20, seed=3), RR.integer_tables(40, 6, 12, 20, seed=3, density=0.25)
    for k in old:
        assert np.array_equal(new[k], old[k]), k
        kept = thin[k] != 0
        assert np.array_equal(thin[k][kept], old[k][kept]), k
        assert not np.signbit(thin[k][~kept]).any(), k
        assert abs(kept.mean() / (old[k] != 0).mean() - 0.25) < 0.1, k


@pytest.mark.parametrize("name", EC.EXACT_NAMES)
def test_exact_cases_are_exact_and_not_trivial(name):
    case = EC.valid_only(EC.exact_case(name))
    tabs, pos, neg, margin, l1 = case
    assert RR.is_exact_step(*case)
    assert margin >= 0
    z = EC.score_diff(tabs, pos, neg, l1) + margin
    assert (z >= 0).any()
    if not name.startswith("dims-1x1"):
        assert (z < 0).any()                                   # the mask matters
    _, g = EC.exact_reference(name)
    for k in tabs:
        assert np.abs(g[k]).max() > 0, k
        # v = g^2 / 4 is checked where |g| < 2^12: on non-zero elements of every table (emap_wrap's few relation
        # rows sum 28,000 pairs each and lie above it)
        small = np.abs(g[k]) < 2.0 ** 12
        assert (g[k][small] != 0).any() or (name.startswith("emap_wrap") and k != "ent"), k


def test_dims_cases_reach_every_instantiation():
    reached = set()
    for name in EC.names("dims"):
        case = EC.exact_case(name)
        pos = case[1]
        assert len(pos) == 224 and len(case[0]["ent"]) == EC.DIMS_E
        assert sorted(np.bincount(pos[:, 2]).tolist()) == sorted(EC.SEGMENTS)
        one = EC.triples_reached(case)
        assert {nc for _, _, nc in one} == {2, 4, 8, 16, 32}, name        # every NC in every case
        reached |= one
    assert reached == EC.ALL_TRIPLES and len(reached) == 20
    dims = {RR.dims(EC.exact_case(n)[0]) for n in EC.names("dims")}
    assert dims == set(EC.DIMS)
    assert any(dr > EC.K_WAVE for _, dr in dims)               # the distance reduction takes several rounds


def test_misaligned_cases_take_vec1_only_when_misaligned():
    for name in EC.names("misaligned"):
        case = EC.exact_case(name)
        assert {v for _, v, _ in EC.triples_reached(case)} == {4}, name
        got = EC.triples_reached(case, aligned=False)
        assert {v for _, v, _ in got} == {1} and {nc for _, _, nc in got} == {2, 4, 8, 16, 32}, name
    assert {EC.exact_case(n)[4] for n in EC.names("misaligned")} == {True, False}


@pytest.mark.parametrize("name", EC.names("tie_and_sign"))
def test_tie_and_sign_conditions(name):
    case = EC.exact_case(name)
    cond = EC.tie_conditions(case)
    assert set(cond) == {"z_zero", "z_minus_one", "u_zero_active", "pos_eq_neg", "h_eq_t"}
    assert all(v >= 1 for v in cond.values()), cond
    tabs, pos, neg, _, _ = case
    assert np.array_equal(pos[EC.TIE_POS_EQ_NEG], neg[EC.TIE_POS_EQ_NEG])
    assert pos[EC.TIE_H_EQ_T, 0] == pos[EC.TIE_H_EQ_T, 1]


@pytest.mark.parametrize("name", EC.names("hot_entity"))
def test_hot_entity_runs(name):
    case = EC.exact_case(name)
    assert len(case[0]["ent"]) == 3 and len(case[1]) == 2000
    assert EC.entity_runs(case).min() > 2000


@pytest.mark.parametrize("name", EC.names("one_pair_per_relation"))
def test_one_pair_per_relation(name):
    tabs, pos, neg, _, _ = EC.exact_case(name)
    R = len(tabs["rel"])
    assert R == len(pos) == 1500 > EC.PLAN_BLOCK               # `base` carries over a pass boundary
    assert np.array_equal(np.sort(pos[:, 2]), np.arange(R)) and np.array_equal(pos[:, 2], neg[:, 2])
    assert set(EC.chunk_sizes(np.bincount(pos[:, 2]))) == {1}


@pytest.mark.parametrize("name", EC.names("key_width"))
def test_key_width_cases(name):
    case = EC.exact_case(name)
    tabs, pos, neg, margin, l1 = case
    E, R = len(tabs["ent"]), len(tabs["rel"])
    assert (E, R) in EC.KEY_WIDTH_ER
    # E and R are powers of two: the sentinel key needs one bit more than the largest id
    assert EC.sort_key_bits(E) == EC.sort_key_bits(E - 1) + 1 and (R == 1 or EC.sort_key_bits(R) == EC.sort_key_bits(R - 1) + 1)
    ok = EC.valid_mask(pos, neg, E, R)
    assert 0.12 <= (~ok).mean() <= 0.18
    ids = np.stack([pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]], 1)
    assert (ids >= E).any(1).sum() >= 10 and (ids < 0).any(1).sum() >= 10 and (pos[:, 2] != neg[:, 2]).sum() >= 10
    vt, vp, vn, _, _ = EC.valid_only(case)
    z = EC.score_diff(vt, vp, vn, l1) + margin
    assert (z < 0).any() and (z >= 0).any()                    # the entity sentinel occurs besides the relation one
    on = z >= 0
    assert max(vp[on, :2].max(), vn[on, :2].max()) == E - 1 and vp[on, 2].max() == R - 1


@pytest.mark.parametrize("name", EC.names("emap_wrap"))
def test_emap_wrap_case(name):
    tabs, pos, _, _, _ = EC.exact_case(name)
    assert 4 * len(pos) > EC.EMAP_WRAP
    assert -(-len(pos) // EC.PLAN_BLOCK) == 137


@pytest.mark.parametrize("which", sorted(EC.ADAM_WRAP))
def test_adam_wrap_cases(which):
    case = EC.adam_wrap_case(which)
    tabs, pos, neg, margin, l1 = case
    assert RR.is_exact_step(*case)
    dim_e, dim_r = RR.dims(tabs)
    vec = EC.vec_for(dim_e, dim_r)
    units = EC.adam_units(tabs, vec)
    over = {k for k, n in units.items() if n > EC.ADAM_UNIT_CAP}
    assert (vec, over) == {"vec1": (1, {"ent", "rel", "rel_matrix"}), "vec4": (4, {"ent", "rel_matrix"})}[which]
    assert max(len(tabs["ent"]), len(tabs["rel"]), len(pos)) > EC.PREP_WRAP          # the prep kernel wraps too
    E, R = len(tabs["ent"]), len(tabs["rel"])
    assert EC.valid_mask(pos, neg, E, R).all() and 60 <= len(pos) <= 70
    assert (EC.score_diff(tabs, pos, neg, l1) + margin >= 0).all()
    ent_rows, rel_rows = EC.adam_wrap_rows(which)
    assert len(ent_rows) == 4 and len(set(rel_rows)) == 4
    assert set(ent_rows) <= set(np.concatenate([pos[:, 0], pos[:, 1], neg[:, 0], neg[:, 1]]).tolist())
    assert set(rel_rows) <= set(pos[:, 2].tolist())
    # the rows straddle the first element of the Adam loop's second round
    for k, rows in (("ent", ent_rows), ("rel_matrix", rel_rows)):
        cols = tabs[k].shape[1]
        assert any(r * cols < EC.ADAM_UNIT_CAP * vec <= (r + 1) * cols for r in rows), k
        assert any(r * cols == EC.ADAM_UNIT_CAP * vec for r in rows), k
    m0, v0 = EC.preset_moments(tabs)
    for k in tabs:
        assert (m0[k] != 0).all() and np.array_equal(v0[k], m0[k] ** 2) and np.array_equal(m0[k] * 8, np.round(m0[k] * 8))


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("dims", EC.FLOAT_DIMS)
def test_float_cases_do_not_hide_behind_the_mask(dims, l1):
    tabs, pos, neg, margin, _ = EC.float_case(dims, l1)
    assert EC.ambiguous_count(tabs, pos, neg, margin, l1) == 0
    on = EC.score_diff(tabs, pos, neg, l1) + margin >= 0
    assert 0.1 * len(pos) <= on.sum() <= 0.9 * len(pos)
    assert margin == float(np.float32(margin))
    for k, x in tabs.items():                                  # what the GPU will hold, and of Xavier's size
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), k
        body = x[:-EC.FAR] if k == "ent" else x
        assert 0.5 < body.std() / np.sqrt(2.0 / sum(x.shape)) < 2.0, k
    far = np.isin(neg[:, 1], np.arange(len(tabs["ent"]) - EC.FAR, len(tabs["ent"])))
    assert far[:len(pos) // 5].all() and (~on[:len(pos) // 5]).mean() > 0.8
