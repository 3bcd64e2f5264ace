"""One TransR training step (ge_transr_adam_step through graphembeddings_amd.transr.TransR) at the edges
test_gpu_transr.py's shapes never reach, on the fixtures of tests/transr_edge_cases.py: every (norm, VEC, NC)
instantiation of the chunk kernel at dims up to 256 x 256, tables and moments off a 16-byte boundary, exact ties and
sign(0), an entity with thousands of gradient slots, one pair per relation, the sorts' key width with both sentinels
present, and every grid-stride loop of the step (score, prep, entity map, Adam) going round more than once.

The exact cases hold small integers, so fp32 computes every intermediate exactly in any order and the loss and the
gradient (read back as m = g / 2 at b1 = 1/2) must equal the fp64 restatement bitwise.  The Adam pass and the steps
from non-integer tables are held to test_gpu_transr.py::test_twenty_dependent_adam_steps's element-wise bounds
(transr_edge_cases.adam_bounds), from inputs the CPU knows.  tests/test_transr_edge_cases_host.py proves the
fixtures are what this file takes them for."""
import numpy as np
import pytest
import torch

from tests import transr_edge_cases as EC
from tests import transr_ref as RR

pytestmark = pytest.mark.gpu
F32_EPS = EC.F32_EPS
TF_B1, TF_B2, TF_EPS = 0.9, 0.999, 1e-8


def _model(tabs, l1):
    from graphembeddings_amd import transr as XR
    dim_e, dim_r = RR.dims(tabs)
    m = XR.TransR(len(tabs["ent"]), len(tabs["rel"]), dim_e, dim_r, l1=l1, seed=0)
    _load(m, tabs)
    return m


def _load(m, tabs, m0=None, v0=None, t=0):
    """Tables, moments (zero if not given) and step count from numpy: a state the CPU knows."""
    for k, x in tabs.items():
        m.tables[k].copy_(torch.as_tensor(np.asarray(x, dtype=np.float32)))
    for buf, mom in ((m.m, m0), (m.v, v0)):
        if mom is None:
            buf.zero_()
        else:
            flat = np.concatenate([np.asarray(mom[k], dtype=np.float32).ravel() for k in RR.TABLES])
            buf.copy_(torch.as_tensor(flat))
    m.t = t


def _off_boundary(t):
    """A copy of t one float past a 16-byte boundary."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view_as(t)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _host(m):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in m.tables.items()}


def _moments(m):
    out = {}
    for k in m.tables:
        a, b = m.moments(k)
        out[k] = (a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
    return out


def _cuda(*xs):
    return [torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in xs]


def _state(m):
    return [m.tables[k].clone() for k in RR.TABLES] + [m.m.clone(), m.v.clone()]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------- exact steps
def _exact_step(name, place=None):
    """One step at b1 = 1/2, b2 = 3/4, t = 1, lr = 2^-6 from zero moments on the whole batch of an exact case,
    checked bitwise against the fp64 gradient of its valid pairs; returns the state after it."""
    tabs, pos, neg, margin, l1 = EC.exact_case(name)
    m = _model(tabs, l1)
    if place == "tables":
        for k in list(m.tables):
            m.tables[k] = _off_boundary(m.tables[k])
    elif place == "moments":
        m.m, m.v = _off_boundary(m.m), _off_boundary(m.v)
    loss = float(m.step(*_cuda(pos, neg), margin, lr=2.0 ** -6, b1=0.5, b2=0.75))
    rloss, g = EC.exact_reference(name)
    assert loss == rloss
    mom = _moments(m)
    for k in tabs:
        mk, vk = mom[k]
        bad = np.argwhere(mk != 0.5 * g[k])
        assert len(bad) == 0, (k, "first (row, col) off:", bad[:4].tolist(), len(bad))
        small = np.abs(g[k]) < 2.0 ** 12
        assert np.array_equal(vk[small], 0.25 * g[k][small] ** 2), k
        assert np.abs(g[k]).max() > 0, k
    return _state(m)


@pytest.mark.parametrize("name", [n for n in EC.EXACT_NAMES if not n.startswith("misaligned-")])
def test_exact_step_bitwise(name):
    _exact_step(name)


@pytest.mark.parametrize("name", EC.names("misaligned"))
def test_misaligned_step_bitwise(name):
    """Tables off a 16-byte boundary, then m and v alone off it: both take VEC 1 where the aligned model takes
    VEC 4, and all three give the fp64 gradient and the same bits."""
    aligned = _exact_step(name)
    assert _same_bits(aligned, _exact_step(name, "tables"))
    assert _same_bits(aligned, _exact_step(name, "moments"))


@pytest.mark.parametrize("name", EC.names("key_width"))
def test_key_width_equals_the_valid_pairs_alone(name):
    """E and R powers of two with both sentinel keys in the sorts: the step equals the step on the valid pairs
    alone, bitwise, in tables, m and v."""
    case = EC.exact_case(name)
    tabs, pos, neg, margin, l1 = case
    _, vp, vn, _, _ = EC.valid_only(case)
    assert len(vp) < len(pos)
    a, b = _model(tabs, l1), _model(tabs, l1)
    la = float(a.step(*_cuda(pos, neg), margin, lr=2.0 ** -6, b1=0.5, b2=0.75))
    lb = float(b.step(*_cuda(vp, vn), margin, lr=2.0 ** -6, b1=0.5, b2=0.75))
    assert la == lb
    assert _same_bits(_state(a), _state(b))


# ------------------------------------------------------------------------------------------- bounded steps
def _bounded_step(label, m, case, m0, v0, t, lr):
    """One step at TF's betas from the loaded state (tables, m0, v0, t - 1): m and v within adam_bounds of the fp64
    step, x recomputed from the GPU's own m and v, the loss within the rounding of its terms."""
    tabs, pos, neg, margin, l1 = case
    dim_e, dim_r = RR.dims(tabs)
    _load(m, tabs, m0, v0, t - 1)
    zero = RR.zeros_like(tabs)
    m0, v0 = m0 or zero, v0 or zero
    loss = float(m.step(*_cuda(pos, neg), margin, lr=lr))
    assert m.t == t
    rloss, g = RR.hinge_grads(tabs, pos, neg, margin, l1)
    _, mag = RR.hinge_grads(tabs, pos, neg, margin, l1, magnitude=True)
    z = EC.score_diff(tabs, pos, neg, l1) + margin
    zmag = RR.score_magnitude(tabs, pos, l1) + RR.score_magnitude(tabs, neg, l1) + abs(margin)
    on = z >= 0
    loss_tol = ((dim_e + dim_r + 8) * 4 * F32_EPS * zmag[on]).sum() + len(pos) * F32_EPS * np.abs(z[on]).sum()
    print(f"{label}: loss error / bound {abs(loss - rloss) / loss_tol:.4f}")
    new, mom = _host(m), _moments(m)
    a = RR.lr_t(*(float(np.float32(x)) for x in (lr, TF_B1, TF_B2)), t)
    bounds = EC.adam_bounds(tabs, m0, v0, g, mag, len(pos), TF_B1, TF_B2)
    worst = {}
    for k in tabs:
        m1, v1 = mom[k]
        mref, mtol, vref, vtol = bounds[k]
        xref = tabs[k] - a * m1 / (np.sqrt(v1) + TF_EPS)
        xtol = 4 * F32_EPS * (np.abs(xref) + a * np.abs(m1) / (np.sqrt(v1) + TF_EPS))
        worst[k] = [float((np.abs(got - ref) / (tol + 1e-300)).max())
                    for got, ref, tol in ((m1, mref, mtol), (v1, vref, vtol), (new[k], xref, xtol))]
        print(f"{label}: {k}: largest error / bound: m {worst[k][0]:.4f}, v {worst[k][1]:.4f}, x {worst[k][2]:.4f}")
    assert abs(loss - rloss) <= loss_tol
    for k, w in worst.items():
        assert max(w) <= 1.0, (k, w)
        assert np.abs(g[k]).max() > 0, k


@pytest.mark.parametrize("which", sorted(EC.ADAM_WRAP))
def test_adam_visits_every_element_once(which):
    """Tables past kAdamMaxBlocks * kBlock units, every element with non-zero m and v before the step: an element
    the grid-stride loop skips or takes twice is off by about lr, thousands of times its bound.  The same step
    from the same state gives the same bits."""
    case = EC.adam_wrap_case(which)
    tabs, _, _, _, l1 = case
    m0, v0 = EC.preset_moments(tabs)
    m = _model(tabs, l1)
    _bounded_step(f"adam_wrap {which}", m, case, m0, v0, EC.ADAM_T, EC.ADAM_LR)
    first = _state(m)
    _load(m, tabs, m0, v0, EC.ADAM_T - 1)
    m.step(*_cuda(case[1], case[2]), case[3], lr=EC.ADAM_LR)
    assert _same_bits(first, _state(m))


@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("dims", EC.FLOAT_DIMS)
def test_step_at_real_dimensions(dims, l1):
    """Xavier-sized tables the CPU knows: step 1 from zero moments, then step 7 from preset non-zero ones."""
    case = EC.float_case(dims, l1)
    tabs = case[0]
    assert EC.ambiguous_count(*case) == 0
    m = _model(tabs, l1)
    label = f"float {dims[0]}x{dims[1]} {'l1' if l1 else 'l2'}"
    _bounded_step(label + " t=1", m, case, None, None, 1, 0.01)
    m0, v0 = EC.preset_moments(tabs)
    _bounded_step(label + " t=7", m, case, m0, v0, 7, 0.01)


def test_large_t():
    """t = 10^6: b1^t and b2^t underflow to 0 in double, so lr_t = lr."""
    case = EC.float_case((12, 8), False)
    assert EC.ambiguous_count(*case) == 0
    assert RR.lr_t(0.01, TF_B1, TF_B2, 10 ** 6) == 0.01
    m0, v0 = EC.preset_moments(case[0])
    _bounded_step("large t", _model(case[0], False), case, m0, v0, 10 ** 6, 0.01)


# ------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("l1", [True, False])
@pytest.mark.parametrize("dims", [(4, 4), (100, 100)])
def test_score_wraps(dims, l1):
    """B = 20,000 > 8,192 waves: the score kernel's grid-stride loop goes round, within test_score_matches_fp64's
    bound."""
    from graphembeddings_amd import transr as XR
    dim_e, dim_r = dims
    E, R, B = 3000, 7, EC.SCORE_B
    m = XR.TransR(E, R, dim_e, dim_r, l1=l1, seed=dim_e)
    tri = RR.skewed_batch(np.random.default_rng(dim_e + dim_r), E, R, B)[0]
    got = m.score(*_cuda(tri)).cpu().numpy().astype(np.float64)
    tabs = _host(m)
    step = 2500                                                # the reference gathers one M_r per triple
    ref = np.concatenate([RR.score(tabs, tri[i:i + step], l1) for i in range(0, B, step)])
    mag = np.concatenate([RR.score_magnitude(tabs, tri[i:i + step], l1) for i in range(0, B, step)])
    tol = (2.0 if l1 else 4.0) * (dim_e + dim_r + 8) * F32_EPS * mag + 1e-30
    print(f"score wrap {dims} {'l1' if l1 else 'l2'}: largest error / bound {(np.abs(got - ref) / tol).max():.4f}")
    assert np.all(np.abs(got - ref) <= tol)
