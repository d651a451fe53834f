"""TEST HELPER — SplattingAvatar's CPU submodule simple_phongsurf and its density control restated in numpy / stock PyTorch:
the reference of every Phong-surface test.

reference (submodules/simple_phongsurf/simple_phongsurf/ unless a path says otherwise):
  * the walk — src/triangle_walk.cpp (cited by line below) behind Triwalk::updateSurfacePointsImpl, src/triangle_walk_py.cpp:62-79.
    float32 / float64 exactly where the C++ has `float` / `double`: `ft` is the type of everything the C++ declares `float`
    (np.float32; np.float64 gives the same walk with every float widened, the yardstick of the position tolerances)
  * the fit — PhongSurfacePy3d.solve_delta_vwd / update_corres_spt / retrieve_vertices / retrieve_normals, phongsurf_py3d.py:151-185,
    :256-327
  * density control — model/baseline/splattingavatar.py `_densify_and_prune` :386-404, `_clone_densify` :407-470, `_split_densify`
    :473-574, `_densification_postfix` :577-603, `_prune` :606-665, `_walking_on_triangles` :668-695, `_reset_opacity` :697-715
The walk cannot be compiled where the fixtures are made (its bundled Eigen is incomplete), so this restatement is held to
answers nobody restated: the straight-line and boundary tests of tests/test_phongsurf_host.py.
`max_radii2D` is left out: `_densification_postfix` zeroes it in clone and in split immediately before the only test that reads it."""
import numpy as np
import torch

PARALLEL_EPS = 1e-7          # :11
MAX_DEPTH = 256              # where the HIP loop stops although the reference would recurse on (status[0])


# ------------------------------------------------------------------------------------------------ the neighbour table
def brute_force_neighbours(faces):
    """initTriangleNeighbor (:176-237) by an O(F^2) search: [F,3] int32, 4 g + k or -1."""
    f = np.asarray(faces).astype(np.int64)
    F = f.shape[0]
    out = np.full((F, 3), -1, np.int32)
    for i in range(F):
        for j in range(3):
            a, b = f[i, j], f[i, (j + 1) % 3]
            for k in range(3):
                hit = np.nonzero((f[:, k] == b) & (f[:, (k + 1) % 3] == a))[0]
                if hit.size:
                    out[i, j] = 4 * hit[0] + k
    return out


# ------------------------------------------------------------------------------------------------ the walk
class Walk:
    """The walk on the mesh whose neighbour table is `nbr` [F,3] (4 g + k or -1).  `status`: the three counters of the HIP
    kernel (crossing cap, resetBaryToInside not settling, point left alone); `trace`: a list that receives every
    signalWalkingPoint."""

    def __init__(self, nbr, decay=0.9, ft=np.float32):
        self.nbr, self.ft, self.decay = np.asarray(nbr), ft, ft(decay)
        self.status = [0, 0, 0]
        self.trace = None

    # :21-28
    def inside(self, b, tol):
        tol = self.ft(tol)
        one = self.ft(1)
        return all(b[k] >= -tol and b[k] <= one + tol for k in range(3))

    # :32-86 — double arithmetic on the float inputs; t12 and the intersection are stored as float
    def intersect(self, p1, p2, p3, p4):
        ft = self.ft
        u1, v1, w1 = (np.float64(x) for x in p1)
        u2, v2, w2 = (np.float64(x) for x in p2)
        u3, v3, w3 = (np.float64(x) for x in p3)
        u4, v4, w4 = (np.float64(x) for x in p4)
        t0 = t1 = ft(0)
        eps = PARALLEL_EPS
        with np.errstate(all="ignore"):
            if abs(u1 - u2) > eps and abs(u4 - u3) > eps:                                     # :45
                if abs(v1 - v2) > eps and abs(v4 - v3) > eps:                                 # :46-51
                    den = (u1 - u2) * (v4 - v3) - (u4 - u3) * (v1 - v2)
                    t0 = ft((u1 * (v4 - v3) + u3 * (v1 - v4) + u4 * (v3 - v1)) / den)
                    t1 = ft((u1 * (v2 - v3) + u2 * (v3 - v1) + u3 * (v1 - v2)) / den)
                elif abs(w1 - w2) > eps and abs(w4 - w3) > eps:                               # :53-58
                    den = (u1 - u2) * (w4 - w3) - (u4 - u3) * (w1 - w2)
                    t0 = ft((u1 * (w4 - w3) + u3 * (w1 - w4) + u4 * (w3 - w1)) / den)
                    t1 = ft((u1 * (w2 - w3) + u2 * (w3 - w1) + u3 * (w1 - w2)) / den)
            elif abs(v1 - v2) > eps and abs(v4 - v3) > eps and abs(w1 - w2) > eps and abs(w4 - w3) > eps:   # :62-69
                den = (v1 - v2) * (w4 - w3) - (v4 - v3) * (w1 - w2)
                t0 = ft((v1 * (w4 - w3) + v3 * (w1 - w4) + v4 * (w3 - w1)) / den)
                t1 = ft((v1 * (w2 - w3) + v2 * (w3 - w1) + v3 * (w1 - w2)) / den)
        if t0 >= 0 and t0 <= 1.0 and t1 >= 0 and t0 <= 1.0:                                   # :72, typo included
            t = np.float64(t0)
            return True, t0, t1, np.array([ft(u1 + t * (u2 - u1)), ft(v1 + t * (v2 - v1)), ft(w1 + t * (w2 - w1))], ft)
        return False, ft(0), ft(0), np.array([ft(u1), ft(v1), ft(w1)], ft)

    def _edge(self, j):
        e0, e1 = np.zeros(3, self.ft), np.zeros(3, self.ft)
        e0[j], e1[(j + 1) % 3] = 1, 1
        return e0, e1

    # :93-113
    def find_crossing_edge(self, p, q):
        for j in range(3):
            _, t0, t1, _ = self.intersect(*self._edge(j), p, q)
            if t0 >= 0.0 and t0 <= 1.0 and np.float64(t1) > 1e-5 and t1 <= 1.0:
                return j
        return -1

    # :120-129
    def find_on_edge(self, p):
        for j in range(3):
            if np.float64(abs(p[j])) < 1e-5:
                return (j + 1) % 3
        return -1

    # :140-147
    def reset_to_zero(self, b, idx):
        ft = self.ft
        v = b[idx]
        b[idx] = 0
        i1, i2 = (idx + 1) % 3, (idx + 2) % 3
        b[i1] = b[i1] + v / ft(2)
        b[i1] = min(max(ft(0), b[i1]), ft(1))
        b[i2] = ft(1) - b[i1]

    # :150-162
    def reset_on_edge(self, b):
        idx, m = 0, b[0]
        for i in (1, 2):
            if abs(b[i]) < abs(m):
                m, idx = b[i], i
        self.reset_to_zero(b, idx)

    # :165-173 (two passes at the most, then clamped and counted: the HIP kernel's status[1])
    def reset_to_inside(self, b):
        for _ in range(2):
            if self.inside(b, 0.0):
                return
            for i in range(3):
                if b[i] < 0:
                    self.reset_to_zero(b, i)
        if self.inside(b, 0.0):
            return
        self.status[1] += 1
        b[0] = min(max(b[0], self.ft(0)), self.ft(1))
        b[1] = min(max(b[1], self.ft(0)), self.ft(1) - b[0])
        b[2] = self.ft(1) - b[0] - b[1]

    def _signal(self, f, b, s):
        if self.trace is not None:
            self.trace.append((int(f), b.copy(), s.copy()))

    # :277-316
    def walk_surface_point(self, f, b, s, depth=0):
        q = b + s
        if self.inside(q, 1e-3):
            b = q.copy()
            self.reset_to_inside(b)
            self._signal(f, b, s)
            return f, b
        if depth >= MAX_DEPTH:
            self.status[0] += 1
            return f, b
        if not self.inside(b, 1e-3):
            if self.find_on_edge(b) == -1:
                b = b.copy()
                self.reset_to_inside(b)
                s = q - b
                self._signal(f, b, s)
                return self.walk_surface_point(f, b, s * self.decay, depth + 1)
        e = self.find_crossing_edge(b, q)
        if e != -1:
            self._signal(f, b, s)
            return self.walk_cross_edge(f, b, s, e, depth)
        e = self.find_on_edge(b)
        if e != -1:
            self._signal(f, b, s)
            return self.walk_cross_edge(f, b, s, e, depth)
        return f, b

    # :318-367 with walkToNeighbor :369-386 and finalize :240-260
    def walk_cross_edge(self, f, b, s, e, depth):
        ft = self.ft
        q = b + s
        ok, _, _, hit = self.intersect(*self._edge(e), b, q)
        if not ok:
            return f, b
        n = int(self.nbr[f, e])
        if n < 0:
            return f, hit
        remain = q - hit
        self._signal(f, hit, remain)
        i_ab = (hit[e], hit[(e + 1) % 3])
        s_ab = (remain[e], remain[(e + 1) % 3])
        n_i, n_s = (i_ab[1], i_ab[0]), (-s_ab[0], -s_ab[1])                      # :382-383
        p = np.array([n_i[0], n_i[1], ft(1) - n_i[0] - n_i[1]], ft)              # :242-245
        qq = np.zeros(3, ft)
        qq[0], qq[1] = p[0] + n_s[0], p[1] + n_s[1]
        qq[2] = ft(1) - qq[0] - qq[1]                                            # :247-250
        sh = qq - p
        g, k = n >> 2, n & 3
        nb, ns = np.zeros(3, ft), np.zeros(3, ft)
        for j in range(3):                                                       # :256-259
            nb[(k + j) % 3], ns[(k + j) % 3] = p[j], sh[j]
        self.reset_on_edge(nb)                                                   # :364
        return self.walk_surface_point(g, nb, ns * self.decay, depth + 1)        # :366

    # triangle_walk_py.cpp:62-79
    def update_surface_points(self, fidx, uv, delta):
        """fidx [n] int, uv [n,2], delta [n,>=2] (the first two columns are read) -> (fidx int32 [n], uv float64 [n,2]): the
        inputs are what the binding receives as doubles; a point whose inputs are not finite or whose face is out of range
        is returned as it came (status[2])."""
        ft = self.ft
        fidx = np.asarray(fidx).astype(np.int32).copy()
        uv = np.asarray(uv).astype(np.float64).copy()
        delta = np.asarray(delta).astype(np.float64)
        F = self.nbr.shape[0]
        for i in range(fidx.shape[0]):
            u, v, du, dv = uv[i, 0], uv[i, 1], delta[i, 0], delta[i, 1]
            if not (0 <= fidx[i] < F) or not np.isfinite([u, v, du, dv]).all():
                self.status[2] += 1
                continue
            b = np.array([ft(u), ft(v), ft(1.0 - ft(u).astype(np.float64) - ft(v).astype(np.float64))], ft)     # :66
            s = np.array([ft(du), ft(dv), ft(0.0 - ft(du).astype(np.float64) - ft(dv).astype(np.float64))], ft)  # :68
            f, b = self.walk_surface_point(int(fidx[i]), b, s)
            fidx[i], uv[i, 0], uv[i, 1] = f, b[0], b[1]
        return fidx, uv


def walk(nbr, fidx, uv, delta, decay=0.9, ft=np.float32):
    """(fidx int32 [n], uv [n,2] as `ft`, status [3]) of one walk."""
    w = Walk(nbr, decay, ft)
    f, uv = w.update_surface_points(fidx, np.asarray(uv, np.float32), np.asarray(delta, np.float32))
    return f, uv.astype(ft), list(w.status)


# ------------------------------------------------------------------------------------------------ the fit
def vertex_normals(verts, faces):
    """Area-weighted vertex normals (pytorch3d's verts_normals_packed): normalize(sum of cross(v2 - v1, v0 - v1)), eps 1e-6."""
    v, f = torch.as_tensor(verts), torch.as_tensor(faces).long()
    t = v[f]
    fn = torch.linalg.cross(t[:, 2] - t[:, 1], t[:, 0] - t[:, 1], dim=1)
    vn = torch.zeros_like(v)
    for k in range(3):
        vn.index_add_(0, f[:, k], fn)
    return torch.nn.functional.normalize(vn, eps=1e-6, dim=1)


def _interp_bary(tri, vw):                                                       # phongsurf_py3d.py:9-14
    bary = torch.concat([vw, 1.0 - vw[..., :1] - vw[..., 1:2]], dim=-1)
    return torch.einsum("nij,ni->nj", tri, bary)


class PhongSurfaceRef:
    """PhongSurfacePy3d with method 'uvd', N = None, max_dist = inf, on tensors of any float dtype; the walk is `Walk`."""

    def __init__(self, V, F, N, outer_loop=2, inner_loop=50, decay=0.9, nbr=None):
        self.V, self.F, self.N = torch.as_tensor(V), torch.as_tensor(F).long(), torch.as_tensor(N)
        self.outer_loop, self.inner_loop, self.decay = outer_loop, inner_loop, decay
        if nbr is None:
            from fateavatar_amd.binding import triangle_neighbours
            nbr = triangle_neighbours(self.F).numpy()
        self.nbr = np.asarray(nbr)
        self.iterations, self.status = [], [0, 0, 0]

    def retrieve_vertices(self, fidx, vw):                                       # :312-320
        return _interp_bary(self.V[self.F[fidx]], vw)

    def retrieve_normals(self, fidx, vw):                                        # :323-327
        return torch.nn.functional.normalize(_interp_bary(self.N[self.F[fidx]], vw), p=2, dim=-1)

    def solve_delta_vwd(self, query, fidx, vw):                                  # :256-309
        delta = torch.full([vw.shape[0], 3], 0.0, dtype=query.dtype)
        delta[:, 2] = (self.retrieve_vertices(fidx, vw) - query).norm(dim=1)
        delta.requires_grad = True
        opt = torch.optim.Adam([delta], lr=0.01)
        last = delta.detach().clone()
        n_it = 0
        for _ in range(self.inner_loop):
            opt.zero_grad()
            cv = self.retrieve_vertices(fidx, vw + delta[:, :2]) * 10
            cn = self.retrieve_normals(fidx, vw + delta[:, :2]) * 10
            loss = torch.nn.functional.mse_loss(cv + cn * delta[:, 2:3], query * 10)
            loss.backward()
            opt.step()
            n_it += 1
            change = (delta - last).norm(dim=1)
            last = delta.detach().clone()
            if (change > 5e-4).sum() == 0:
                break
        self.iterations.append(n_it)
        return delta.detach()

    def triwalk_update(self, fidx, vw, delta, ft=np.float32):                    # :72-85
        w = Walk(self.nbr, self.decay, ft)
        f, uv = w.update_surface_points(fidx.numpy(), vw.numpy(), delta.numpy())
        self.status = [a + b for a, b in zip(self.status, w.status)]
        return torch.from_numpy(f).to(fidx.dtype), torch.from_numpy(uv).to(vw.dtype)

    def update_corres_spt(self, query, N, fidx, vw):                             # :151-185
        assert N is None
        for _ in range(self.outer_loop):
            with torch.enable_grad():
                d = self.solve_delta_vwd(query, fidx, vw)
            fidx, vw = self.triwalk_update(fidx, vw, d[:, :2])
        return fidx, vw


# ------------------------------------------------------------------------------------------------ density control
NAMES = ("_uvd", "_opacity", "_features_dc", "_features_rest", "_rotation", "_scaling")   # train/optim.py:106-117


def build_rotation(r):                                                           # tools/gs_utils/general_utils.py:78-99
    q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


class SplattingRef:
    """SplattingAvatar's Gaussians as six nn.Parameters in one Adam (one group each), the embedding (`sample_fidxs`,
    `sample_bary`) and the densification statistics.  `surf`: a PhongSurfaceRef of the canonical mesh; `mesh_verts`: the posed
    vertices of the last frame (:490-493)."""
    percent_dense = 0.01

    def __init__(self, params, fidxs, bary, surf, mesh_verts, lrs=None):
        self.p = {n: torch.nn.Parameter(params[n].detach().clone()) for n in NAMES}
        lrs = lrs or {}
        self.opt = torch.optim.Adam([dict(params=[self.p[n]], lr=float(lrs.get(n, 1e-3)), name=n) for n in NAMES], lr=0.0)
        self.sample_fidxs, self.sample_bary = fidxs.detach().clone().long(), bary.detach().clone()
        self.surf, self.mesh_verts = surf, mesh_verts
        self._postfix()

    @property
    def P(self):
        return int(self.sample_fidxs.shape[0])

    def step(self, grads):
        for n in NAMES:
            self.p[n].grad = grads[n].detach().clone().reshape(self.p[n].shape)
        self.opt.step()

    def moments(self, n):
        st = self.opt.state.get(self.p[n])
        return (None, None) if not st else (st["exp_avg"], st["exp_avg_sq"])

    def _postfix(self):                                                          # :598-603
        self.xyz_gradient_accum = torch.zeros((self.P, 1))
        self.denom = torch.zeros((self.P, 1))

    def _replace(self, group, new, moments=None):
        old = group["params"][0]
        stored = self.opt.state.get(old, None)
        new = torch.nn.Parameter(new)
        if stored is not None:
            stored["exp_avg"], stored["exp_avg_sq"] = moments(stored["exp_avg"]), moments(stored["exp_avg_sq"])
            del self.opt.state[old]
            self.opt.state[new] = stored
        group["params"][0] = new
        self.p[group["name"]] = new

    def _cat(self, ext, fidxs, bary):                                            # :445-470, :546-571, :577-603
        for group in self.opt.param_groups:
            add = ext[group["name"]]
            self._replace(group, torch.cat((group["params"][0].detach(), add), dim=0),
                          lambda m, add=add: torch.cat((m, torch.zeros_like(add)), dim=0))
        self.sample_fidxs = torch.cat([self.sample_fidxs, fidxs.long()], dim=0)
        self.sample_bary = torch.cat([self.sample_bary, bary], dim=0)
        self._postfix()

    def prune(self, mask):                                                       # :606-665
        valid = ~mask
        for group in self.opt.param_groups:
            self._replace(group, group["params"][0].detach()[valid], lambda m: m[valid])
        self.sample_fidxs, self.sample_bary = self.sample_fidxs[valid], self.sample_bary[valid]
        self.xyz_gradient_accum, self.denom = self.xyz_gradient_accum[valid], self.denom[valid]
        return int(mask.sum())

    def clone_densify(self, grads, max_grad, extent):                            # :407-470
        sel = torch.norm(grads, dim=-1) >= max_grad
        sel = sel & (torch.max(torch.exp(self.p["_scaling"].detach()), dim=1).values <= self.percent_dense * extent)
        self._cat({n: self.p[n].detach()[sel] for n in NAMES}, self.sample_fidxs[sel], self.sample_bary[sel])
        return int(sel.sum())

    def split_densify(self, grads, max_grad, extent, generator=None, N=2):       # :473-574
        padded = torch.zeros(self.P)
        padded[:grads.shape[0]] = grads.squeeze(-1)
        scaling, rotation, uvd = (self.p[n].detach() for n in ("_scaling", "_rotation", "_uvd"))
        sel = (padded >= max_grad) & (torch.max(torch.exp(scaling), dim=1).values > self.percent_dense * extent)
        stds = torch.exp(scaling)[sel].repeat(N, 1)
        samples = torch.normal(mean=torch.zeros((stds.size(0), 3)), std=stds, generator=generator)
        rots = build_rotation(torch.nn.functional.normalize(rotation[sel])).repeat(N, 1, 1)
        F = self.surf.F
        tri = lambda a: a[F[self.sample_fidxs]]  # noqa: E731
        base_xyz = torch.einsum("nij,ni->nj", tri(self.mesh_verts), self.sample_bary)                     # :490-493
        base_n = torch.nn.functional.normalize(torch.einsum("nij,ni->nj", tri(self.surf.N), self.sample_bary), dim=-1)
        xyz_cano = base_xyz + base_n * uvd[..., -1:]
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + xyz_cano[sel].repeat(N, 1)
        fidx, uv = self.sample_fidxs[sel].repeat(N), self.sample_bary[sel, :2].repeat(N, 1)
        d = uvd[sel, -1:].repeat(N, 1)
        self.new_xyz = new_xyz
        if fidx.numel():
            fidx, uv = self.surf.update_corres_spt(new_xyz, None, fidx, uv)                               # :517
        ext = {"_uvd": torch.concat([torch.zeros_like(uv), d], dim=-1),
               "_scaling": torch.log(torch.exp(scaling)[sel].repeat(N, 1) / (0.8 * N)),
               "_rotation": rotation[sel].repeat(N, 1),
               "_features_dc": self.p["_features_dc"].detach()[sel].repeat(N, 1, 1),
               "_features_rest": self.p["_features_rest"].detach()[sel].repeat(N, 1, 1),
               "_opacity": self.p["_opacity"].detach()[sel].repeat(N, 1)}
        self._cat(ext, fidx, torch.concat([uv, 1.0 - uv[:, 0:1] - uv[:, 1:2]], dim=-1))
        n = int(sel.sum())
        self.prune(torch.cat((sel, torch.zeros(N * n, dtype=torch.bool))))
        return n

    def densify_and_prune(self, max_grad=2e-4, min_opacity=0.005, extent=2.0, max_screen_size=None, generator=None):   # :386-404
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        n_clone = self.clone_densify(grads, max_grad, extent)
        n_split = self.split_densify(grads, max_grad, extent, generator)
        mask = (torch.sigmoid(self.p["_opacity"].detach()) < min_opacity).squeeze(-1)
        if max_screen_size:
            mask = mask | (torch.exp(self.p["_scaling"].detach()).max(dim=1).values > 0.1 * extent)
        return n_clone, n_split, self.prune(mask)

    def walk_on_triangles(self):                                                 # :668-695
        uvd = self.p["_uvd"].detach()
        w = Walk(self.surf.nbr, self.surf.decay)
        fidx, uv = w.update_surface_points(self.sample_fidxs.numpy(), self.sample_bary[:, :2].numpy(), uvd[:, :2].numpy())
        self.walk_status = list(w.status)
        self.sample_fidxs = torch.tensor(fidx).long()
        self.sample_bary[..., :2] = torch.tensor(uv).float()
        self.sample_bary[..., 2] = 1.0 - self.sample_bary[..., 0] - self.sample_bary[..., 1]
        for group in self.opt.param_groups:
            if group["name"] == "_uvd":
                def zero_uv(m):
                    m[..., :2] = 0
                    return m
                self._replace(group, torch.cat((torch.zeros_like(uvd[..., :2]), uvd[..., 2:]), dim=-1), zero_uv)

    def reset_opacity(self):                                                     # :697-715
        old = self.p["_opacity"].detach()
        new = torch.min(torch.sigmoid(old), torch.ones_like(old) * 0.01)
        new = torch.log(new / (1 - new))
        for group in self.opt.param_groups:
            if group["name"] == "_opacity":
                self._replace(group, new, torch.zeros_like)


# ------------------------------------------------------------------------------------------------ the known-answer lattice
SHEAR = np.array([[1.0, 0.3], [0.2, 0.9]])


def sheared_lattice(n=6):
    """n x n unit squares, all split along the same diagonal, sheared by SHEAR: (verts2d [(n+1)^2, 2] float64, faces [2 n^2, 3]
    int32).  Every neighbour of a triangle is its point reflection about the shared edge's midpoint, so the reference's edge
    transfer (swap a, b; negate the shift) continues a straight line exactly when decay is 1."""
    gx, gy = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    grid = np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1).astype(np.float64)
    faces = []
    for y in range(n):
        for x in range(n):
            v00, v10, v11, v01 = y * (n + 1) + x, y * (n + 1) + x + 1, (y + 1) * (n + 1) + x + 1, (y + 1) * (n + 1) + x
            faces += [(v00, v10, v11), (v00, v11, v01)]
    return grid @ SHEAR.T, np.array(faces, np.int32)


def _locate(p, n):
    """Face and barycentrics (float64) of the unsheared point p inside the n x n lattice."""
    x, y = int(np.floor(p[0])), int(np.floor(p[1]))
    fx, fy = p[0] - x, p[1] - y
    sq = 2 * (y * n + x)
    if fx >= fy:     # (v00, v10, v11): p = v00 + (fx - fy) e_x... in barycentrics (1 - fx, fx - fy, fy)
        return sq, np.array([1 - fx, fx - fy, fy])
    return sq + 1, np.array([1 - fy, fx, fy - fx])      # (v00, v11, v01)


def lattice_walks(seed, count, n=6, max_cross=8, margin=0.03, leave=False):
    """`count` seeded straight walks on the sheared lattice: dict of fidx [count] int32, uv [count,2] float32, delta [count,2]
    float32, crossings [count] (lattice lines crossed), start / end [count,2] float64 (2-D positions, the end the EXACT one for
    the float32 inputs: start + du (V0 - V2) + dv (V1 - V2)), first [count] (the parameter t of the first crossing, 1 if none).
    Start, end and every crossing keep `margin` (in barycentric units) from edges / lattice vertices, so that no tolerance
    branch of the walk (isBaryInside's 1e-3, findOnEdgeIndex's 1e-5) is in play.  `leave`: the end lies OUTSIDE the lattice
    instead; `end` is then where the segment meets the boundary."""
    rng = np.random.default_rng(seed)
    verts, faces = sheared_lattice(n)
    inv = np.linalg.inv(SHEAR)
    out = {k: [] for k in ("fidx", "uv", "delta", "crossings", "start", "end", "first")}
    per = {c: 0 for c in range(max_cross + 1)}
    want = -(-count // (max_cross + 1))
    while len(out["fidx"]) < count:
        a = rng.uniform(0.1, n - 0.1, 2)
        b = rng.uniform(-3.0, n + 3.0, 2) if leave else a + rng.normal(0, 1.0, 2) * rng.uniform(0.05, 2.5)
        inside_b = bool((b > 0.1).all() and (b < n - 0.1).all())
        if inside_b == leave:
            continue
        f, bary = _locate(a, n)
        if bary.min() < margin:
            continue
        uv = bary[:2].astype(np.float32)
        tri = verts[faces[f]]
        E = np.stack([tri[0] - tri[2], tri[1] - tri[2]], axis=1)                      # 2 x 2: columns d/du, d/dv
        delta = np.linalg.solve(E, SHEAR @ (b - a)).astype(np.float32)
        # the exact walk of the ROUNDED inputs
        start = uv[0].astype(np.float64) * tri[0] + uv[1].astype(np.float64) * tri[1] + (1 - np.float64(uv[0]) - np.float64(uv[1])) * tri[2]
        end = start + E @ delta.astype(np.float64)
        a2, b2 = inv @ start, inv @ end
        d = b2 - a2
        ts = []
        for num, den in ((lambda k: k - a2[0], d[0]), (lambda k: k - a2[1], d[1]), (lambda k: k - (a2[0] - a2[1]), d[0] - d[1])):
            if abs(den) < 1e-3:
                ts = None     # (nearly parallel to a family of lattice lines: skipped)
                break
            for k in range(-n - 4, 2 * n + 5):
                t = num(k) / den
                if 0 < t < 1:
                    ts.append(t)
        if ts is None:
            continue
        ts = sorted(ts)
        if leave:
            exits = [t for t in ((0 - a2[0]) / d[0], (n - a2[0]) / d[0], (0 - a2[1]) / d[1], (n - a2[1]) / d[1]) if 0 < t < 0.9]
            if not exits:
                continue
            t_out = min(exits)
            ts = [t for t in ts if t <= t_out + 1e-12]
            end, b2 = start + t_out * (end - start), a2 + t_out * d
        pts = [a2 + t * d for t in ts]
        if any(np.abs(p - np.round(p)).max() < margin for p in pts):                  # a crossing too close to a lattice vertex
            continue
        if len(ts) > 1 and np.diff(ts).min() * np.linalg.norm(d) < margin:            # two crossings too close to each other
            continue
        c = len(ts) - (1 if leave else 0)
        if not leave:
            if c > max_cross or per[c] >= want or _locate(b2, n)[1].min() < margin:
                continue
            if c == 1 and _locate(a2 + (ts[0] + 0.9 * (1 - ts[0])) * d, n)[1].min() < margin:
                continue
            per[c] += 1
        elif c > 2 * max_cross:
            continue
        for k, v in zip(out, (f, uv, delta, c, start, end, ts[0] if ts else 1.0)):
            out[k].append(v)
    return {k: np.array(v, {"fidx": np.int32, "crossings": np.int32}.get(k)) for k, v in out.items()}


def lattice_position(verts2d, faces, fidx, uv):
    """2-D positions (float64) of surface points on the lattice."""
    tri = verts2d[faces[np.asarray(fidx)]]
    uv = np.asarray(uv, np.float64)
    return uv[:, :1] * tri[:, 0] + uv[:, 1:2] * tri[:, 1] + (1 - uv[:, :1] - uv[:, 1:2]) * tri[:, 2]


# ------------------------------------------------------------------------------------------------ shared inputs
def position(V, F, fidx, uv):
    """3-D positions (float64) of surface points on the mesh (V, F)."""
    tri = np.asarray(V, np.float64)[np.asarray(F)[np.asarray(fidx)]]
    uv = np.asarray(uv, np.float64)
    return uv[:, :1] * tri[:, 0] + uv[:, 1:2] * tri[:, 1] + (1 - uv[:, :1] - uv[:, 1:2]) * tri[:, 2]


def template_walk_inputs(n_faces, n=4096):
    """The walk test's inputs on the template: `n` seeded points, deltas uniform in +-0.5 for the first half and exactly zero
    for the second: (fidx int32 [n], uv float32 [n,2], delta float32 [n,2])."""
    from fateavatar_amd.splatting import sample_bary_on_triangles
    fidx, bary = sample_bary_on_triangles(n_faces, n, torch.Generator().manual_seed(3))
    delta = (torch.rand(n, 2, generator=torch.Generator().manual_seed(4)) - 0.5).numpy().astype(np.float32)
    delta[n // 2:] = 0
    return fidx.numpy().astype(np.int32), bary[:, :2].contiguous().numpy(), delta
