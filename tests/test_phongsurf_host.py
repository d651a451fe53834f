"""CPU: the references of the Phong-surface tests (tests/phongsurf_ref.py) held to answers nobody restated, and the host-side
neighbour table.

  (a) the restated solve reproduces every case of tests/golden/golden_phongsurf.npz (the reference's own solve_delta_vwd),
      iteration counts included.  `n8_long` (inner_loop 500) stopped after 79 iterations: an intermediate global stop IS pinned.
  (b) `binding.triangle_neighbours` against a brute-force search, its symmetry, its boundary count
  (c) the restated walk against the straight line on the sheared lattice (decay 1), and the 0.9 decay of one crossing
  (d) a walk that leaves the lattice ends on the boundary at the intersection point
  (e) every walked point is valid and no counter of the walk is set
  (f) the restated density control on a 12-Gaussian state whose selections are worked out by hand
"""
import os

import numpy as np
import pytest
import torch

from fateavatar_amd.binding import triangle_neighbours
from tests import phongsurf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["n96_s4", "n3000_s05", "n3000_s4", "n3000_s20", "n65_surface", "n8_long"]


@pytest.fixture(scope="module")
def template():
    g = np.load(os.path.join(ROOT, "fateavatar_amd", "data", "head_template_geom.npz"))
    V, F = torch.from_numpy(g["verts"]).float(), torch.from_numpy(g["faces"]).long()
    return V, F, R.vertex_normals(V, F)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_phongsurf.npz"))


@pytest.fixture(scope="module")
def lattice():
    verts, faces = R.sheared_lattice()
    return verts, faces, triangle_neighbours(torch.from_numpy(faces)).numpy()


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("case", CASES)
def test_restated_solve_reproduces_the_fixture(template, golden, case):
    V, F, N = template
    s = R.PhongSurfaceRef(V, F, N, 1, int(golden[case + "_inner"]), nbr=np.zeros((1, 3), np.int32))
    d = s.solve_delta_vwd(torch.from_numpy(golden[case + "_query"]), torch.from_numpy(golden[case + "_fidx"]).long(),
                          torch.from_numpy(golden[case + "_uv"]))
    assert s.iterations == [int(golden[case + "_iters"])]
    assert np.array_equal(d.numpy(), golden[case + "_delta"])      # the same torch operations: the same bits


def test_fixture_pins_what_its_notes_say(golden):
    assert int(golden["n65_surface_iters"]) == 1 and not golden["n65_surface_delta"].any()
    assert 1 < int(golden["n8_long_iters"]) < 500 and "an intermediate global stop is pinned" in str(golden["notes"][0])
    # the 1 / 3n of the loss: the same 96 points move differently alone and inside the batch of 3 000
    assert np.array_equal(golden["n96_s4_query"], golden["n3000_s4_query"][:96])
    bound = 4 * np.abs(golden["n96_s4_delta"].astype(np.float64) - golden["n96_s4_delta64"]).max()
    assert np.abs(golden["n96_s4_delta"] - golden["n3000_s4_delta"][:96]).max() > bound


# ---------------------------------------------------------------------------------------------------------------- (b)
def test_neighbour_table_on_a_lattice(lattice):
    _, faces, nbr = lattice
    grid4 = R.sheared_lattice(4)[1]
    n4 = triangle_neighbours(torch.from_numpy(grid4)).numpy()
    assert n4.dtype == np.int32 and np.array_equal(n4, R.brute_force_neighbours(grid4))
    assert int((n4 < 0).sum()) == 16 and int((nbr < 0).sum()) == 24


def test_neighbour_table_on_the_template(template):
    _, F, _ = template
    nbr = triangle_neighbours(F).numpy()
    f = F.numpy()
    assert nbr.shape == (10006, 3) and int((nbr < 0).sum()) == 30
    rows = np.random.default_rng(5).choice(f.shape[0], 500, replace=False)
    for i in rows:
        for j in range(3):
            a, b = f[i, j], f[i, (j + 1) % 3]
            want = -1
            for k in range(3):
                hit = np.nonzero((f[:, k] == b) & (f[:, (k + 1) % 3] == a))[0]
                if hit.size:
                    want = 4 * hit[0] + k
            assert nbr[i, j] == want
    fi, ej = np.nonzero(nbr >= 0)
    back = nbr[nbr[fi, ej] >> 2, nbr[fi, ej] & 3]
    assert np.array_equal(back >> 2, fi) and np.array_equal(back & 3, ej)       # symmetric


def test_neighbour_table_rejects_a_repeated_directed_edge():
    with pytest.raises(ValueError):
        triangle_neighbours(torch.tensor([[0, 1, 2], [0, 1, 3]]))
    assert triangle_neighbours(torch.zeros((0, 3), dtype=torch.int64)).shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------- (c)
def _valid(fidx, uv, F):
    return bool((fidx >= 0).all() and (fidx < F).all() and (uv >= 0).all() and (uv.sum(axis=1) <= 1).all())


def test_walk_is_a_straight_line_on_the_sheared_lattice(lattice):
    verts, faces, nbr = lattice
    w = R.lattice_walks(1, 200)
    assert set(np.unique(w["crossings"])) == set(range(9))
    fidx, uv, status = R.walk(nbr, w["fidx"], w["uv"], w["delta"], decay=1.0)
    err = np.linalg.norm(R.lattice_position(verts, faces, fidx, uv) - w["end"], axis=1)
    assert err.max() <= 1e-5, (err.max(), w["crossings"][err.argmax()])          # of the unit cell
    assert status == [0, 0, 0] and _valid(fidx, uv, faces.shape[0])


def test_one_crossing_keeps_nine_tenths_of_what_lies_beyond_the_edge(lattice):
    verts, faces, nbr = lattice
    w = R.lattice_walks(1, 200)
    one = w["crossings"] == 1
    assert one.sum() >= 20
    fidx, uv, status = R.walk(nbr, w["fidx"][one], w["uv"][one], w["delta"][one], decay=0.9)
    s, e, t = w["start"][one], w["end"][one], w["first"][one][:, None]
    cross = s + t * (e - s)
    err = np.linalg.norm(R.lattice_position(verts, faces, fidx, uv) - (cross + 0.9 * (e - cross)), axis=1)
    assert err.max() <= 1e-5 and status == [0, 0, 0] and _valid(fidx, uv, faces.shape[0])


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_walk_that_leaves_the_lattice_stops_on_the_boundary(lattice):
    verts, faces, nbr = lattice
    w = R.lattice_walks(2, 60, leave=True)
    fidx, uv, status = R.walk(nbr, w["fidx"], w["uv"], w["delta"], decay=1.0)
    err = np.linalg.norm(R.lattice_position(verts, faces, fidx, uv) - w["end"], axis=1)
    assert err.max() <= 1e-5 and status == [0, 0, 0]
    assert _valid(fidx, np.maximum(uv, 0), faces.shape[0]) and uv.min() > -1e-6
    assert (nbr[fidx] < 0).any(axis=1).all()                                     # a boundary face


# ---------------------------------------------------------------------------------------------------------------- (e)
def test_template_walk_is_valid_and_widening_the_floats_moves_nothing(template):
    """The inputs of the GPU test on the template: no counter is set, every result is valid, and the restatement with every
    float widened to double ends within nanometres — the yardstick profiles/r14_phongsurf.md records."""
    V, F, _ = template
    fidx, uv, delta = R.template_walk_inputs(int(F.shape[0]))
    nbr = triangle_neighbours(F).numpy()
    f32, u32, s32 = R.walk(nbr, fidx, uv, delta)
    f64, u64, s64 = R.walk(nbr, fidx, uv, delta, ft=np.float64)
    assert s32 == [0, 0, 0] and s64 == [0, 0, 0] and _valid(f32, u32, int(F.shape[0]))
    d = np.linalg.norm(R.position(V, F, f32, u32) - R.position(V, F, f64, u64), axis=1)
    p99 = np.percentile(d, 99)
    print(f"float32 vs widened walk: p99 {p99:.3e} max {d.max():.3e} over 4 x p99: {(d > 4 * p99).mean():.4f}")
    assert (d > 4 * p99).mean() <= 0.01
    still = (delta == 0).all(axis=1) & (np.minimum(uv.min(axis=1), 1 - uv.sum(axis=1)) > 1e-3)
    assert still.sum() > 1500 and np.array_equal(u32[still], uv[still]) and np.array_equal(f32[still], fidx[still])


# ---------------------------------------------------------------------------------------------------------------- (f)
def _hand_state(template):
    """12 Gaussians on the template.  extent 2 -> the clone / split threshold on max exp(_scaling) is 0.02.
    row:        0     1     2     3     4     5     6     7     8     9    10    11
    grad     3e-4  3e-4  1e-4  3e-4  1e-4  3e-4  3e-4  1e-4  2e-4   0    3e-4  3e-4     (>= 2e-4 selects)
    scale    0.01  0.03  0.01  0.05  0.03  0.019 0.01  0.05  0.021  0.01 0.01  0.04
    opacity  0.5   0.5   0.5   0.5   0.5   0.5   0.001 0.5   0.5    0.5  0.5   0.001
    clone: grad and scale <= 0.02 -> rows 0, 5, 6, 10 (4).  split: grad and scale > 0.02 -> rows 1, 3, 8, 11 (4; row 8's
    gradient is exactly the threshold).  After the clone P = 16, after the split 16 + 8 - 4 = 20.  Final prune: opacity
    0.001 -> row 6, its clone, and the two children of row 11 (4) -> P = 16."""
    V, F, N = template
    g = torch.Generator().manual_seed(12)
    P = 12
    grad = torch.tensor([3e-4, 3e-4, 1e-4, 3e-4, 1e-4, 3e-4, 3e-4, 1e-4, 2e-4, 0, 3e-4, 3e-4])
    scale = torch.tensor([0.01, 0.03, 0.01, 0.05, 0.03, 0.019, 0.01, 0.05, 0.021, 0.01, 0.01, 0.04])
    opacity = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.001, 0.5, 0.5, 0.5, 0.5, 0.001])
    from fateavatar_amd.splatting import sample_bary_on_triangles
    fidxs, bary = sample_bary_on_triangles(int(F.shape[0]), P, g)
    params = {"_uvd": torch.cat([torch.zeros(P, 2), 0.001 * torch.arange(1, P + 1).float()[:, None]], dim=1),
              "_opacity": torch.log(opacity / (1 - opacity))[:, None], "_features_dc": torch.rand(P, 1, 3, generator=g),
              "_features_rest": torch.zeros(P, 0, 3), "_rotation": torch.nn.functional.normalize(torch.randn(P, 4, generator=g)),
              "_scaling": torch.log(scale)[:, None] * torch.ones(1, 3) - torch.tensor([0.0, 0.1, 0.2])}
    ref = R.SplattingRef(params, fidxs, bary, R.PhongSurfaceRef(V, F, N, 2, 50), V + 0.002, lrs={n: 0.0 for n in R.NAMES})
    ref.step({n: 0.01 * torch.randn(params[n].shape, generator=g) for n in R.NAMES})        # rate 0: non-zero moments, values untouched
    ref.xyz_gradient_accum = 2 * grad[:, None].clone()
    ref.denom = torch.full((P, 1), 2.0)
    ref.denom[9] = 0                                                                        # 0 / 0 -> NaN -> 0
    return ref, params, fidxs, bary


def test_restated_density_control_on_a_hand_made_state(template):
    ref, params, fidxs, bary = _hand_state(template)
    m_before = ref.moments("_scaling")[0].clone()
    counts = ref.densify_and_prune(max_grad=2e-4, min_opacity=0.005, extent=2.0, generator=torch.Generator().manual_seed(1))
    assert counts == (4, 4, 4) and ref.P == 16
    assert ref.surf.status == [0, 0, 0] and len(ref.surf.iterations) == 2
    # survivors, in order: rows 0 2 4 5 7 9 10 (6 pruned; 1 3 8 11 split away), clones of 0 5 10 (6's pruned), children of 1 3 8 twice
    keep = [0, 2, 4, 5, 7, 9, 10]
    uvd = ref.p["_uvd"].detach()
    assert torch.equal(uvd[:7], params["_uvd"][keep]) and torch.equal(uvd[7:10], params["_uvd"][[0, 5, 10]])
    assert torch.equal(ref.sample_fidxs[7:10], fidxs[[0, 5, 10]]) and torch.equal(ref.sample_bary[7:10], bary[[0, 5, 10]])
    assert torch.equal(uvd[10:, 2], params["_uvd"][[1, 3, 8, 1, 3, 8], 2]) and not uvd[:, :2].any()    # the parent's d; (u, v) zero
    assert torch.allclose(ref.p["_scaling"].detach()[10:], torch.log(torch.exp(params["_scaling"][[1, 3, 8, 1, 3, 8]]) / 1.6))
    b = ref.sample_bary[10:]
    assert (b >= 0).all() and torch.allclose(b.sum(dim=1), torch.ones(6)) and (ref.sample_fidxs >= 0).all()
    m, v = ref.moments("_scaling")
    assert torch.equal(m[:7], m_before[keep]) and not m[7:].any() and not v[7:].any()                  # zero moments on new rows
    assert not ref.xyz_gradient_accum.any() and not ref.denom.any() and ref.denom.shape == (16, 1)
    # the children lie near their parent: the fit moved them on the canonical mesh by less than a few standard deviations
    child = ref.surf.retrieve_vertices(ref.sample_fidxs[10:], b[:, :2])
    parent = ref.surf.retrieve_vertices(fidxs[[1, 3, 8, 1, 3, 8]], bary[[1, 3, 8, 1, 3, 8], :2])
    assert ((child - parent).norm(dim=1) < 0.25).all()


def test_restated_walk_and_opacity_reset_on_the_hand_made_state(template):
    ref, params, fidxs, bary = _hand_state(template)
    ref.walk_on_triangles()                      # (u, v) of _uvd are zero: nobody moves
    assert ref.walk_status == [0, 0, 0]
    assert torch.equal(ref.sample_fidxs, fidxs) and torch.equal(ref.sample_bary[:, :2], bary[:, :2])
    with torch.no_grad():
        ref.p["_uvd"][:, 0] = 0.3
        ref.p["_uvd"][:, 1] = -0.2
    ref.walk_on_triangles()
    uvd, (m, v) = ref.p["_uvd"].detach(), ref.moments("_uvd")
    assert not uvd[:, :2].any() and torch.equal(uvd[:, 2], params["_uvd"][:, 2])
    assert not m[:, :2].any() and not v[:, :2].any() and m[:, 2].all() and v[:, 2].all()
    assert not torch.equal(ref.sample_bary[:, :2], bary[:, :2])
    assert (ref.sample_bary >= -1e-6).all() and torch.allclose(ref.sample_bary.sum(dim=1), torch.ones(12))
    ref.reset_opacity()
    op = torch.sigmoid(ref.p["_opacity"].detach()).reshape(-1)
    want = torch.tensor([0.01] * 6 + [0.001] + [0.01] * 4 + [0.001])
    assert torch.allclose(op, want, rtol=1e-5)
    m, v = ref.moments("_opacity")
    assert not m.any() and not v.any() and ref.moments("_scaling")[0].all()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """No GPU needed: every refusal, and the n == 0 no-op, return before a launch."""
    import ctypes as C
    from fateavatar_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(64)          # never dereferenced on these paths
    fit = lambda n, outer, inner, ptr=p: L.fr_phong_fit(None, ptr, ptr, ptr, ptr, 4, 4, n, ptr, ptr, ptr, outer, inner, 0.9, ptr, ptr, None)  # noqa: E731
    for outer, inner in ((0, 50), (9, 50), (2, 0), (2, 513)):
        assert fit(8, outer, inner) == _lib.FR_ERR_INVALID_ARGUMENT and "fr_phong_fit" in _lib.last_error()
    assert fit(8, 2, 50, None) == _lib.FR_ERR_INVALID_ARGUMENT and fit(-1, 2, 50) == _lib.FR_ERR_INVALID_ARGUMENT
    assert fit(0, 2, 50, None) == _lib.FR_OK and fit(0, 8, 512) == _lib.FR_OK
    walk = lambda n, ptr=p, stride=2: L.fr_triwalk(None, ptr, 4, n, ptr, ptr, ptr, stride, 0.9, ptr)  # noqa: E731
    assert walk(8, None) == _lib.FR_ERR_INVALID_ARGUMENT and walk(8, p, 1) == _lib.FR_ERR_INVALID_ARGUMENT
    assert walk(-1) == _lib.FR_ERR_INVALID_ARGUMENT and walk(0, None) == _lib.FR_OK


def test_phong_surface_refuses_what_is_not_built():
    from fateavatar_amd.phongsurf import PhongSurface
    import simple_phongsurf
    assert simple_phongsurf.PhongSurfacePy3d is PhongSurface
    V, F = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]])
    N = torch.tensor([[0.0, 0, 1]] * 3)
    with pytest.raises(NotImplementedError):
        PhongSurface(V, F, N, method="uv")
    with pytest.raises(ValueError):
        PhongSurface(V, F, N, inner_loop=513)
    s = PhongSurface(V, F, N)
    assert (s.outer_loop, s.inner_loop, s.method) == (4, 500, "uvd") and s.faces_nbr.tolist() == [[-1, -1, -1]]
    with pytest.raises(NotImplementedError):
        s.update_corres_spt(V, N, torch.zeros(3, dtype=torch.long), torch.zeros(3, 2))
    assert torch.allclose(s.retrieve_vertices(torch.tensor([0]), torch.tensor([[0.25, 0.5]])), torch.tensor([[0.5, 0.25, 0.0]]))
    assert not hasattr(s, "find_corres_spt") and not hasattr(s, "init_corres_spt")
