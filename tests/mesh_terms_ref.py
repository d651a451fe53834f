"""TEST HELPER — FateAvatar's mesh terms restated in stock PyTorch on DENSE matrices, with a dtype argument (float64 is what
the kernel tests are held to, float32 what the step tests add to the image term):
  * `laplacian_dense` — pytorch3d 0.7.7's `Meshes.laplacian_packed().to_dense()` (pytorch3d.ops.laplacian, the uniform
    Laplacian) by its rule, written independently of `binding.mesh_laplacian` (a python set of edges, no sorting tricks):
    the edges are the unique undirected pairs {a, b}, a != b, among the faces' sides; L[i,j] = 1 / deg(i) for a neighbour j,
    L[i,i] = -1 for EVERY vertex.  pytorch3d is not installed here: the rule is pinned by the hand-written matrices of
    tests/test_mesh_terms_host.py, not by a run of pytorch3d.
  * `laplacian_smoothing`, `flame_distance` — the expressions of FateAvatarLoss (train/loss.py:112-121, :192-197), pinned by
    tests/test_reference_runs_host.py to recorded runs of the class's own `get_laplacian_smoothing_loss` and
    `accumulate_gradients` with `laplacian_matrix` preset to `laplacian_dense` (tests/golden/reference_image_terms.npz, case
    `fate`): what the reference does WITH the matrix is recorded, the matrix rule is not.
  * what the GPU tests need around them: float64 values / gradients / rounding magnitudes, and the seeded inputs;
  * `float64_terms_sparse` — the same dictionary from gathers and `index_add_` over the edge list, for meshes whose V x V matrix
    does not fit (pinned to `float64_terms` by tests/test_mesh_terms_host.py), and `random_mesh_drawn_at_once` for such meshes."""
import numpy as np
import torch


def laplacian_dense(faces, V, dtype=torch.float64):
    edges = set()
    for tri in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                edges.add((min(a, b), max(a, b)))
    A = torch.zeros((V, V), dtype=dtype)
    for a, b in edges:
        A[a, b] = A[b, a] = 1
    deg = A.sum(1)
    L = torch.where(deg[:, None] > 0, A * (1.0 / deg)[:, None], torch.zeros_like(A))   # (1.0 / deg, then the product: :laplacian)
    L[torch.arange(V), torch.arange(V)] = -1
    return L


def laplacian_smoothing(L, verts_orig, verts):
    """get_laplacian_smoothing_loss(verts_orig, verts): [V,3] or [1,V,3] vertices, `L` [V,V]."""
    L = L[None, ...].detach()
    vo, v = verts_orig.reshape(1, -1, 3), verts.reshape(1, -1, 3)
    basis = L.bmm(vo).detach()
    moved = L.bmm(v)
    return ((moved - basis) ** 2).sum(dim=-1, keepdim=True).mean()


def flame_distance(verts_orig, verts):
    return ((verts - verts_orig) ** 2).mean()


def float64_terms(faces, V, verts_orig, verts, w_lap, w_flame):
    """Float64 truth of one fr_mesh_terms launch on float32 inputs, with the magnitudes its rounding bounds are written in:
    dict(lap, flame: the losses; grad [V,3]: w_lap dlap/dverts + w_flame dflame/dverts; r, d [V,3]; Mr = |L| |d|,
    Mg = (2/V) |L|^T Mr, deg [V])."""
    L = laplacian_dense(faces, V, torch.float64)
    vo = verts_orig.double()
    v = verts.double().clone().requires_grad_(True)
    lap, fl = laplacian_smoothing(L, vo, v), flame_distance(vo, v)
    (w_lap * lap + w_flame * fl).backward()
    d = (v.detach() - vo)
    Mr = L.abs() @ d.abs()
    return dict(lap=lap.item(), flame=fl.item(), grad=v.grad, r=L @ d, d=d, Mr=Mr, Mg=(2.0 / max(V, 1)) * (L.abs().T @ Mr),
                deg=(L > 0).sum(1))


def float64_terms_sparse(faces, V, verts_orig, verts, w_lap, w_flame):
    """`float64_terms` without the V x V matrix.  The directed edges (i, j) come from numpy's `unique` over the faces' sides in
    both directions (neither `laplacian_dense`'s python set nor `binding.mesh_laplacian`); with s_i = sum_{j in N(i)} x_j as an
    `index_add_` over them,  (L x)_i = s_i(x) / deg_i - x_i,  (|L| x)_i = s_i(x) / deg_i + x_i,  and, the adjacency being
    symmetric,  (|L|^T x)_i = s_i(x / deg) + x_i."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2], f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 0], f[:, 1], f[:, 2]])
    keep = a != b
    pairs = np.unique(a[keep] * V + b[keep])
    row, col = torch.from_numpy(pairs // V), torch.from_numpy(pairs % V)
    deg = torch.bincount(row, minlength=V)
    inv = torch.where(deg > 0, 1.0 / deg.double().clamp_min(1), torch.zeros(V, dtype=torch.float64))

    def nsum(x):                                   # s_i(x), [V, k]
        return torch.zeros_like(x).index_add_(0, row, x[col])

    vo = verts_orig.double()
    v = verts.double().clone().requires_grad_(True)
    r = nsum(v - vo) * inv[:, None] - (v - vo)
    lap, fl = (r ** 2).sum(dim=-1, keepdim=True).mean(), ((v - vo) ** 2).mean()
    (w_lap * lap + w_flame * fl).backward()
    d = v.detach() - vo
    Mr = nsum(d.abs()) * inv[:, None] + d.abs()
    Mg = (2.0 / max(V, 1)) * (nsum(Mr * inv[:, None]) + Mr)
    return dict(lap=lap.item(), flame=fl.item(), grad=v.grad, r=r.detach(), d=d, Mr=Mr, Mg=Mg, deg=deg)


def random_mesh_drawn_at_once(V, seed):
    """`random_mesh`'s distribution (V random vertices, 2 V faces of three distinct random indices) from two calls of the
    generator instead of 2 V: index triples are drawn with repeats and the rows with a repeat dropped.  Other draws than
    `random_mesh(V, seed)`; for the sizes at which that one takes minutes."""
    g = np.random.default_rng(seed)
    verts = g.standard_normal((V, 3)).astype(np.float32) * 0.1
    tri = g.integers(0, V, (2 * V + 64, 3))
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    assert tri.shape[0] >= 2 * V
    return verts, tri[:2 * V].astype(np.int64)


def random_mesh(V, seed):
    """V random vertices and 2 V faces of three distinct random indices (none for V < 3): irregular degrees, repeated
    edges and, at some seeds, vertices no face uses."""
    g = np.random.default_rng(seed)
    verts = g.standard_normal((V, 3)).astype(np.float32) * 0.1
    if V < 3:
        return verts, np.zeros((0, 3), np.int64)
    faces = np.stack([g.choice(V, 3, replace=False) for _ in range(2 * V)]).astype(np.int64)
    return verts, faces


def displaced(verts, seed):
    """verts_orig = `verts`; verts = verts_orig + a smooth 1 cm displacement + 1 mm noise (float32 numpy)."""
    g = np.random.default_rng(seed + 1000)
    smooth = 0.01 * np.stack([np.sin(7.0 * verts[:, 1] + 0.3), np.cos(5.0 * verts[:, 2]), np.sin(6.0 * verts[:, 0] - 0.2)], 1)
    return (verts + smooth + 0.001 * g.standard_normal(verts.shape)).astype(np.float32)
