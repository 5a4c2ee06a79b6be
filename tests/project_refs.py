"""Scenes and a float64 reference of the projection (csrc/project.hip, project_fwd_body.hpp, project_common.hpp, project_bwd.hip) for
tests/test_gpu_project_edges.py.  No GPU: tests/test_project_refs_host.py runs all of it on exactly the GPU test's inputs, checks the
backward against finite differences of the forward and measures the constants at the end of this file with the fp32 C oracle.

The reference is oracle/torch_ref.py::project in float64 under autograd (tests/test_oracle_vs_torch_ref.py uses it for the whole
pipeline), evaluated PER (camera, Gaussian) PAIR -- torch.func.vmap over the pairs, every pair with its own copy of its Gaussian and its
camera -- so that the gradient of every pair is available on its own, the camera's included.  What the C ABI adds is restated here:
  opac_eff      = opacity x compensation (antialiased) or opacity (classic); its cotangent v_opac_eff feeds v_opacities and, times the
                  opacity, the compensation's cotangent;
  sums          over the cameras for v_means / v_quats / v_scales / v_opacities, over the Gaussians for v_viewmats;
  x_quat_rows / x_mean_rows  addends of v_quats / v_means;
  compensation  gsplat's add_blur_vjp divides by comp + 1e-6 where autograd divides by comp; the VJP is linear in the compensation's
                  cotangent, which is therefore scaled by comp / (comp + 1e-6).  comp > 0 in every scene (asserted by the host test);
                  comp == 0 has a case of its own, flat_case, compared with the C oracle;
  wire rows     v_rgb passes where 0 <= x + 0.5 <= 1 (torch.clamp's rule) or where the row's clamp bit is set;
  raw rows      blend_refs.rows_to_dense, the restatement of project_bwd.hip::rows_to_gradients.

Sums of |terms| (the scale of every tolerance, as in blend_refs): the VJP is linear in the eight cotangent components of a pair
(v_means2d 2, v_depths 1, v_conics 3, v_compensations 1, v_opac_eff 1).  `derivatives` returns the gradient of every output per UNIT of
each component (seven one-hot autograd passes: the last two components share the compensation's); a reference number is
sum_j v_j d_j over the components and the cameras (and the Gaussians, for v_viewmats), its terms sum_j |v_j| |d_j|, plus |addend| for the
x_* rows.  Errors are measured in units of 2^-24 x terms with blend_refs.worst_ratio.

Generator limits (what keeps the problem well conditioned; test_project_refs_host.py asserts what they promise):
  depth 2 .. 10 in front of every camera (near plane 0.01: far inside), eps2d = 0.3, opacities 0.05 .. 0.95, cameras within 0.03 rad
  and 0.05 units of the first;
  scales 0.03 .. 0.4, any two axes of a Gaussian a factor 1.4 .. 5.8 apart: between two equal axes a rotation changes nothing and the
  quaternion's gradient is a difference of equal numbers;
  quaternions of norm 0.2 .. 5 (the kernels normalise; none near zero) in a random direction, but no principal axis within
  acos(0.85) = 32 degrees of a viewing ray: the extent along the ray does not move the footprint in first order, its scale's gradient is
  1e-5 of the other two and every float32 evaluation rounds it away (measured with the C oracle before the limit: 26 000 x 2^-24 terms);
  more generally the elements of ONE gradient share their roundings (the rotation matrix, the covariance), so an element is known to
  2^-24 of its largest sibling, not of itself: a direction is redrawn while the terms of the elements of a pair's quaternion or scale
  gradient are more than a factor MAX_SIBLING = 16 apart (this scene's cotangents, antialiased and classic).  A condition on the
  float64 reference alone.
  Of every 12 consecutive Gaussians six lie outside the 1.3 x tan-fov clamp: x+, x-, y+, y-, x+ y+, x- y-,
  at 1.15 .. 1.6 times the limit; the others stay below 0.8 times: nothing within 1e-3 of a limit, where torch's minimum would split the
  gradient at a tie.
"""
import functools

import numpy as np
import torch

from oracle import torch_ref as tr
from tests import blend_refs as B

F = np.float32
EPS2D = 0.3
W, H = 160, 96
MAX_SIBLING = 16.0                   # terms of the largest over the smallest element of one quaternion or scale gradient, at the most
MAX_AXIS_RAY = 0.85                  # |cos| between a principal axis and a viewing ray, at the most
COMP_EPS = 1e-6                      # project_common.hpp kCompEps, gsplat add_blur_vjp
NEAR, FAR = 0.01, 1e10
CLAMP_GROUPS = {0: (1, 0), 1: (-1, 0), 2: (0, 1), 3: (0, -1), 4: (1, 1), 5: (-1, -1)}      # n % 12 -> side of x, y outside the clamp
COMPONENTS = ("means2d_x", "means2d_y", "depth", "conic_a", "conic_b", "conic_c", "comp")      # (+ opac_eff: through `comp` and v_opacities)
OUTPUTS = ("means", "quats", "scales", "opacities", "viewmat")


def _rot(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rotmat(q):
    """[n, 3, 3] of wxyz quaternions of any norm (oracle/torch_ref.py::quat_to_rotmat in numpy)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


def axis_ray(quats, rays):
    """[n]: the largest |cosine| between a principal axis of Gaussian n and one of its viewing rays (rays [C, n, 3], unit, world)."""
    return np.abs(np.einsum("nij,cni->cnj", rotmat(quats), rays)).max(axis=(0, 2))


def limits(K):
    """lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg of persp_proj for one K (float64)."""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    tx, ty = 0.5 * W / fx, 0.5 * H / fy
    return (W - cx) / fx + 0.3 * tx, cx / fx + 0.3 * tx, (H - cy) / fy + 0.3 * ty, cy / fy + 0.3 * ty


def _cotangents(C, N, seed):
    """Random float32 cotangents for every pair: v_means2d [C,N,2], v_depths [C,N], v_conics [C,N,3], v_comp [C,N], v_opac_eff [C,N]."""
    r = np.random.RandomState(seed)
    shape = (C, N)
    return dict(v_means2d=r.standard_normal(shape + (2,)).astype(F), v_depths=r.standard_normal(shape).astype(F),
                v_conics=(r.standard_normal(shape + (3,)) * 10).astype(F), v_comp=r.standard_normal(shape).astype(F),
                v_opac_eff=r.standard_normal(shape).astype(F))


class Scene:
    """N Gaussians in front of C cameras of W x H pixels, float32 arrays; `masks`: name -> bool [C, N], the radii > 0 pattern a
    backward call is given (the tests dictate it: every Gaussian here projects in every camera)."""

    def __init__(self, name, C, N, seed):
        self.name, self.C, self.N = name, C, N
        r = np.random.RandomState(seed)
        K0 = np.array([[0.9 * W, 0, W / 2 + 3.5], [0, 0.95 * W, H / 2 - 2.25], [0, 0, 1]])
        R0 = _rot(r.standard_normal(3), 0.3)
        t0 = np.array([0.1, -0.2, 0.3])
        vms, Ks = [], []
        for c in range(C):
            Rc = _rot(r.standard_normal(3), r.uniform(0.005, 0.03)) @ R0 if c else R0
            tc = t0 + (r.uniform(-0.05, 0.05, 3) if c else 0.0)
            vm = np.eye(4)
            vm[:3, :3], vm[:3, 3] = Rc, tc
            vms.append(vm)
            Ks.append(K0 * np.array([[1 + 0.01 * (c % 5), 1, 1], [1, 1 - 0.01 * (c % 3), 1], [1, 1, 1]]))
        self.viewmats, self.Ks = np.array(vms).astype(F), np.array(Ks).astype(F)
        lxp, lxn, lyp, lyn = limits(K0)
        z = r.uniform(2.0, 10.0, N)
        ux, uy = r.uniform(-0.8, 0.8, N), r.uniform(-0.8, 0.8, N)
        xz = np.where(ux >= 0, ux * lxp, ux * lxn)
        yz = np.where(uy >= 0, uy * lyp, uy * lyn)
        self.group = np.full(N, -1)
        for n in range(N):
            g = CLAMP_GROUPS.get(n % 12)
            if g is None:
                continue
            self.group[n] = n % 12
            if g[0]:
                xz[n] = g[0] * r.uniform(1.15, 1.6) * (lxp if g[0] > 0 else lxn)
            if g[1]:
                yz[n] = g[1] * r.uniform(1.15, 1.6) * (lyp if g[1] > 0 else lyn)
        cam = np.stack([xz * z, yz * z, z], axis=1)
        self.means = ((cam - t0) @ R0).astype(F)                        # R0^T (cam - t0)
        # scales: base x (1, r1, r1 r2) in a random order, r1 and r2 in 1.4 .. 2.4
        r1, r2 = r.uniform(1.4, 2.4, N), r.uniform(1.4, 2.4, N)
        mult = np.stack([np.ones(N), r1, r1 * r2], axis=1)
        mult = np.take_along_axis(mult, np.argsort(r.uniform(size=(N, 3)), axis=1), axis=1)
        self.scales = (r.uniform(0.03, 0.069, N)[:, None] * mult).astype(F)
        # quaternions: a random direction, redrawn while a principal axis lies within acos(MAX_AXIS_RAY) of a camera's viewing ray
        rays = np.einsum("cij,nj->cni", np.array(vms)[:, :3, :3], self.means.astype(np.float64)) + np.array(vms)[:, None, :3, 3]
        rays = np.einsum("cji,cnj->cni", np.array(vms)[:, :3, :3], rays / np.linalg.norm(rays, axis=-1, keepdims=True))      # world frame
        # ... and while an element of the quaternion's or the scale's gradient of some camera has less than 1 / MAX_SIBLING of the
        # terms of its largest sibling (with this scene's cotangents, both modes)
        self.opac = r.uniform(0.05, 0.95, N).astype(F)
        self.cot = _cotangents(C, N, seed + 1000)
        q, norms = np.zeros((N, 4)), r.uniform(0.2, 5.0, (N, 1))
        todo = np.ones(N, bool)
        while todo.any():
            inner = todo.copy()
            while inner.any():
                q[inner] = r.standard_normal((int(inner.sum()), 4))
                q[inner] /= np.linalg.norm(q[inner], axis=1, keepdims=True)
                inner &= axis_ray(q, rays) > MAX_AXIS_RAY
            self.quats = (q * norms).astype(F)
            idx = np.flatnonzero(todo)
            todo[idx] = self.sibling_ratio(idx) > MAX_SIBLING
        self.masks = self._masks(r)

    def sibling_ratio(self, idx):
        """[len(idx)]: over the cameras, the quaternion and the scale gradient and both modes, the largest ratio between the terms of
        the largest and of the smallest element of one gradient of Gaussian idx[k]."""
        idx = np.asarray(idx)
        pc, pn = (v.reshape(-1) for v in np.meshgrid(np.arange(self.C), idx, indexing="ij"))
        d = derivatives(self.means, self.quats, self.scales, self.viewmats, self.Ks, pc, pn)
        worst = np.zeros(pc.size)
        c = self.cot
        for aa in (True, False):
            _, M = cotangent_matrix(d, self.opac, c["v_means2d"], c["v_depths"], c["v_conics"], c["v_comp"], c["v_opac_eff"], aa)
            for key in ("quats", "scales"):
                T = (M[:, :, None] * np.abs(d[key])).sum(axis=1)
                worst = np.maximum(worst, T.max(axis=1) / T.min(axis=1))
        return worst.reshape(self.C, idx.size).max(axis=0)

    def _masks(self, r):
        C, N = self.C, self.N
        m = {"none": np.zeros((C, N), bool), "all": np.ones((C, N), bool), "mixed": r.uniform(size=(C, N)) < 0.3}
        for k in (0, 63, 64, 255, N - 1):                               # exactly one visible pair: thread k of block 0, the last Gaussian
            if k < N:
                one = np.zeros((C, N), bool)
                one[C - 1, k] = True
                m[f"one@{k}"] = one
        if N >= 256:                                                    # waves 0-2 of block 0 empty, wave 3 full
            w3 = np.zeros((C, N), bool)
            w3[:, 192:256] = True
            m["wave3"] = w3
        if C > 1:
            cam = np.zeros((C, N), bool)
            cam[C // 2] = True
            m["one-camera"] = cam
        return m


# name: (cameras, Gaussians, seed).  N on both sides of the 256-thread block, N = 1301 is no multiple of 4, 64 or 256, C on both sides of
# the 64 camera slots of project_bwd_kernel and twice beyond them.
_SPECS = {"c1-n1": (1, 1, 1), "c1-n255": (1, 255, 2), "c2-n256": (2, 256, 3), "c3-n257": (3, 257, 4), "c1-n600": (1, 600, 5),
          "c2-n600": (2, 600, 6), "c65-n257": (65, 257, 7), "c130-n70": (130, 70, 8), "c1-n1301": (1, 1301, 9)}
SCENES = tuple(_SPECS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return Scene(name, *_SPECS[name])


# ---- forward ------------------------------------------------------------------------------------------------------------------------
FWD_MARGIN = 1e-5       # a radius or a cull comparison closer than this (relative) to its threshold in float64 is not compared
MAX_EXCLUDED = 0.01     # of the pairs of a scene


def forward(means, quats, scales, viewmats, Ks, eps2d=EPS2D, near=NEAR, far=FAR, radius_clip=0.0):
    """oracle/torch_ref.py::project in float64 on float32 inputs -> dict of numpy arrays radii[C,N] int64, means2d, depths, conics,
    comp (unculled values everywhere) and `critical`[C,N]: the pre-ceil radius or one of the cull comparisons (near, far, the four
    screen edges) lies within FWD_MARGIN of its threshold."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    radii, m2, z, con, comp = tr.project(t(means), t(quats), t(scales), t(viewmats), t(Ks), W, H, eps2d=eps2d, near=near, far=far,
                                         radius_clip=radius_clip)
    radii, m2, z, con, comp = (v.numpy() for v in (radii, m2, z, con, comp))
    a, b, c = con[..., 0], con[..., 1], con[..., 2]
    with np.errstate(all="ignore"):
        idet = a * c - b * b                                            # the blurred covariance is the conic's inverse
        c00, c11, det = c / idet, a / idet, 1.0 / idet
        mid = 0.5 * (c00 + c11)
        rpre = 3.0 * np.sqrt(mid + np.sqrt(np.maximum(0.01, mid * mid - det)))
        rad = np.ceil(rpre)
        near_ = lambda v, thr, scale: np.abs(v - thr) <= FWD_MARGIN * scale
        crit = near_(rpre, np.round(rpre), rpre) | near_(z, near, abs(near)) | near_(z, far, abs(far))      # (radius <= radius_clip compares the ceiled integer: exact once the radius is)
        for v, thr in ((m2[..., 0] + rad, 0.0), (m2[..., 0] - rad, W), (m2[..., 1] + rad, 0.0), (m2[..., 1] - rad, H)):
            crit |= near_(v, thr, np.abs(v - rad) + rad + abs(thr))
    return dict(radii=radii, means2d=m2, depths=z, conics=con, comp=comp, critical=crit | ~np.isfinite(rpre))


def forward_terms(sc_means, viewmats, Ks, fwd):
    """Sums of |terms| of the forward's float outputs: means2d = fx x / z + cx; depth = <R row, m> + t; a conic entry is a covariance
    entry over det = c00 c11 - c01^2.  The entries of J Sigma J^T are sums of signed products as large as the covariance's trace (a thin
    Gaussian seen edge-on), and the determinant is a difference that cancels for an elongated splat: (c00 + c11) / det x
    (c00 c11 + c01^2) / det for all three; the compensation sqrt(det_orig / det) takes the second factor."""
    m = np.asarray(sc_means, dtype=np.float64)
    vm, K = np.asarray(viewmats, dtype=np.float64), np.asarray(Ks, dtype=np.float64)
    zt = np.abs(vm[:, None, 2, :3] * m[None]).sum(-1) + np.abs(vm[:, None, 2, 3])
    m2 = fwd["means2d"]
    cxy = np.stack([K[:, 0, 2], K[:, 1, 2]], axis=-1)[:, None, :]
    m2t = (np.abs(m2 - cxy) + np.abs(cxy)) * (zt / np.abs(fwd["depths"]))[..., None]
    con = fwd["conics"]
    a, b, c = con[..., 0], con[..., 1], con[..., 2]
    cond = (a * c + b * b) / (a * c - b * b)
    return dict(means2d=m2t, depths=zt, conics=np.repeat(((a + c) * cond)[..., None], 3, axis=-1), comp=fwd["comp"] * cond)


# ---- backward -------------------------------------------------------------------------------------------------------------------------
def derivatives(means, quats, scales, viewmats, Ks, pc, pn, eps2d=EPS2D, comp_in=None):
    """The pairs (camera pc[p], Gaussian pn[p]): gradient of each of the seven outputs of COMPONENTS with respect to the pair's own
    mean [P,7,3], quaternion [P,7,4], scale [P,7,3] and camera [P,7,4,4], in float64; plus the pair's compensation [P] and the
    compensation's derivative already scaled by comp / (comp + 1e-6) (gsplat's add_blur_vjp).  comp_in [P]: the compensations the
    backward call is given; the seventh derivative is then gsplat's formula with exactly those, through the gradient of comp^2 -- the
    only form that exists at comp == 0, where autograd's sqrt has no derivative."""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    pc, pn = np.asarray(pc, dtype=np.int64), np.asarray(pn, dtype=np.int64)
    leaves = [t(means)[pn].clone().requires_grad_(True), t(quats)[pn].clone().requires_grad_(True),
              t(scales)[pn].clone().requires_grad_(True), t(viewmats)[pc].clone().requires_grad_(True)]
    Kp = t(Ks)[pc]
    P = pc.size
    if P == 0:
        return dict(means=np.zeros((0, 7, 3)), quats=np.zeros((0, 7, 4)), scales=np.zeros((0, 7, 3)), viewmat=np.zeros((0, 7, 4, 4)),
                    comp=np.zeros(0), pc=pc, pn=pn)

    def one(m, q, s, v, k):
        _, m2, z, con, comp = tr.project(m[None], q[None], s[None], v[None], k[None], W, H, eps2d=eps2d)
        # det_orig / det = comp^2 from the conic (the blurred covariance is its inverse): differentiable where comp is 0
        a, b, c = con.reshape(3).unbind(0)
        det = 1.0 / (a * c - b * b)
        ratio = ((c * det - eps2d) * (a * det - eps2d) - (b * det) ** 2) / det
        if comp_in is not None:
            comp = comp.detach()                                        # (sqrt at 0: 0 x inf in the backward pass)
        return torch.cat([m2.reshape(2), z.reshape(1), con.reshape(3), comp.reshape(1), ratio.reshape(1), (c * det).reshape(1),
                          (-b * det).reshape(1), (a * det).reshape(1)])      # (... and the blurred covariance c00, c01, c11)

    out = torch.func.vmap(one)(*leaves, Kp)                             # [P, 8]
    comp = out[:, 6].detach()
    grads = [[] for _ in leaves]
    for j in range(7):
        hot = torch.zeros_like(out)
        if j < 6:
            hot[:, j] = 1.0
        elif comp_in is None:
            hot[:, 6] = comp / (comp + COMP_EPS)
        else:      # the compensation the call is GIVEN (float32, possibly 0): add_blur_vjp is 0.5 / (comp + 1e-6) times the gradient of comp^2
            comp = t(comp_in)
            hot[:, 7] = 0.5 / (comp + COMP_EPS)
        for dst, g in zip(grads, torch.autograd.grad(out, leaves, grad_outputs=hot, retain_graph=True)):
            dst.append(g.numpy())
    d = {k: np.stack(g, axis=1) for k, g in zip(("means", "quats", "scales", "viewmat"), grads)}
    d.update(comp=comp.numpy(), pc=pc, pn=pn, conics=out[:, 3:6].detach().numpy())
    if comp_in is not None:      # the derivatives of the covariance's three entries: name -> [P, 3, .], for the terms of flat_case
        cov = [[] for _ in leaves]
        for j in (8, 9, 10):
            hot = torch.zeros_like(out)
            hot[:, j] = 1.0
            for dst, g in zip(cov, torch.autograd.grad(out, leaves, grad_outputs=hot, retain_graph=True)):
                dst.append(g.numpy())
        d["cov"] = {k: np.stack(g, axis=1) for k, g in zip(("means", "quats", "scales", "viewmat"), cov)}
    return d


def cotangent_matrix(d, opac, v_means2d, v_depths, v_conics, v_comp, v_opac_eff, antialiased, mags=None):
    """[P, 7] float64: the cotangent of each output of COMPONENTS for the pairs of `d`, from [C, N, .] arrays (None = absent);
    `mags` (same layout, optional): the magnitudes that stand in for |cotangent| in the terms."""
    pc, pn = d["pc"], d["pn"]
    g = lambda a: np.asarray(a, dtype=np.float64)[pc, pn]
    V = np.zeros((pc.size, 7))
    V[:, 0:2], V[:, 2], V[:, 3:6] = g(v_means2d), g(v_depths), g(v_conics)
    M = np.abs(V) if mags is None else np.concatenate([g(mags["means2d"]), g(mags["depths"])[:, None], g(mags["conics"]), np.zeros((pc.size, 1))], 1)
    if antialiased:
        o = np.asarray(opac, dtype=np.float64)[pn]
        if v_comp is not None:
            V[:, 6] += g(v_comp)
            M[:, 6] += np.abs(g(v_comp))
        if v_opac_eff is not None:
            V[:, 6] += g(v_opac_eff) * o
            M[:, 6] += np.abs(g(v_opac_eff) * o)
    return V, M


def backward(C, N, d, V, M, opac=None, v_opac_eff=None, antialiased=True, x_quat=None, x_mean=None):
    """name -> (value, terms) for means [N,3], quats [N,4], scales [N,3], opacities [N] (with v_opac_eff), viewmat [C,4,4].
    x_quat [N,4] / x_mean [N,3]: dense forms of the x_quat_rows / x_mean_rows addends."""
    pc, pn = d["pc"], d["pn"]
    out = {}
    for name, idx, n in (("means", pn, N), ("quats", pn, N), ("scales", pn, N), ("viewmat", pc, C)):
        D = d[name]
        ex = (slice(None), slice(None)) + (None,) * (D.ndim - 2)
        val, trm = np.zeros((n,) + D.shape[2:]), np.zeros((n,) + D.shape[2:])
        np.add.at(val, idx, (V[ex] * D).sum(axis=1))
        np.add.at(trm, idx, (M[ex] * np.abs(D)).sum(axis=1))
        out[name] = [val, trm]
    for name, x in (("quats", x_quat), ("means", x_mean)):
        if x is not None:
            out[name][0] += np.asarray(x, dtype=np.float64)
            out[name][1] += np.abs(np.asarray(x, dtype=np.float64))
    if v_opac_eff is not None:
        voe = np.asarray(v_opac_eff, dtype=np.float64)[pc, pn] * (d["comp"] if antialiased else 1.0)
        val, trm = np.zeros(N), np.zeros(N)
        np.add.at(val, pn, voe)
        np.add.at(trm, pn, np.abs(voe))
        out["opacities"] = [val, trm]
    return {k: tuple(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def scene_derivatives(name, mask):
    sc = scene(name)
    pc, pn = np.nonzero(sc.masks[mask])
    return derivatives(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, pc, pn)


@functools.lru_cache(maxsize=None)
def scene_forward(name):
    """The float64 forward of a scene and its float32 roundings: the conics and compensations a backward call is given."""
    sc = scene(name)
    f = forward(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks)
    f["conics32"], f["comp32"] = f["conics"].astype(F), f["comp"].astype(F)
    return f


def cotangents(name):
    return scene(name).cot


def reference(name, mask, antialiased=True, with_vcomp=True, with_voe=True, cot=None, x_quat=None, x_mean=None):
    """The reference of one backward call on a scene: name -> (value, terms)."""
    sc = scene(name)
    cot = cot or cotangents(name)
    d = scene_derivatives(name, mask)
    V, M = cotangent_matrix(d, sc.opac, cot["v_means2d"], cot["v_depths"], cot["v_conics"], cot["v_comp"] if with_vcomp else None,
                            cot["v_opac_eff"] if with_voe else None, antialiased)
    return backward(sc.C, sc.N, d, V, M, sc.opac, cot["v_opac_eff"] if with_voe else None, antialiased, x_quat, x_mean)


# ---- raw-moment rows and wire rows --------------------------------------------------------------------------------------------------------
class _Rows:
    """What blend_refs.rows_to_dense reads of a scene."""

    def __init__(self, conics, opac):
        self.conics, self.opac = np.asarray(conics), np.asarray(opac)


def raw_to_gradients(rows, conics, o_eff):
    """The documented meaning of converted rows: [v_xy 2 | |v_xy| 2 | v_conic 3 | v_opacity_eff] from the raw moments (float64), and
    the magnitudes of the sums inside: |v_x| <= o (|a m1| + |b m2|), the scale its float32 rounding is measured against."""
    rows = np.asarray(rows, dtype=np.float64)
    g = B.rows_to_dense(_Rows(conics, o_eff), rows[:, :8])
    o = np.abs(np.asarray(o_eff, dtype=np.float64))
    a, b, c = (np.abs(np.asarray(conics, dtype=np.float64)[:, k]) for k in range(3))
    mag = np.abs(g)
    mag[:, 0] = o * (a * np.abs(rows[:, 0]) + b * np.abs(rows[:, 1]))
    mag[:, 1] = o * (b * np.abs(rows[:, 0]) + c * np.abs(rows[:, 1]))
    return g, mag


def clamp_pass(x_plus_half):
    """torch.clamp(x + 0.5, 0, 1)'s backward mask."""
    v = np.asarray(x_plus_half)
    return (v >= 0) & (v <= 1)


# ---- the compact path's inputs (C = 1, one gradient row per visible Gaussian) ---------------------------------------------------------------
BIG = "c1-n1301"                     # N is no multiple of 4 or 256
NVIS = (1, 255, 256, 257, 513)       # rows: one, a block less one, a block, a block and one, two blocks and one


@functools.lru_cache(maxsize=None)
def compact_case(n_vis):
    """n_vis visible Gaussians of the large scene with culled ones between them and one compact gradient row for each -- the scene's own
    cotangents: 40 % of the rows zero in everything, five rows non-zero through exactly one of v_depths, v_compensations,
    v_opac_eff, x_quat_rows, x_mean_rows.  -> ids [n_vis] int32 (increasing), rows: name -> float32 [n_vis, .], zero [n_vis] bool, the
    derivatives of the pairs, `only`: row -> its single input."""
    sc = scene(BIG)
    r = np.random.RandomState(n_vis)
    ids = np.sort(r.choice(sc.N, n_vis, replace=False)).astype(np.int32)
    rows = {k: np.array(v[0, ids], dtype=np.float64) for k, v in sc.cot.items()}
    rows.update(x_quat=r.standard_normal((n_vis, 4)), x_mean=r.standard_normal((n_vis, 3)), x_abs=r.uniform(0.1, 1, (n_vis, 2)),
                x_col=r.standard_normal((n_vis, 12)))
    zero = r.uniform(size=n_vis) < 0.4
    # the single-input rows: v_compensations and v_opac_eff alone on the two rows where the compensation's own VJP is best conditioned
    # -- (1 - comp^2) conic - eps2d det(conic) cancels as comp -> 1 (measured with the C oracle at comp 0.99: 560 x 2^-24 terms) and
    # the sibling limit of the scene speaks of whole rows: the smallest spread between the elements of the compensation's derivative
    # with respect to mean, quaternion and scale, over 1 - comp^2 --, the others on the first rows that are left
    d = derivatives(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, np.zeros(n_vis, np.int64), ids)
    spread = np.max([np.abs(d[k][:, 6]).max(axis=1) / np.abs(d[k][:, 6]).min(axis=1) for k in ("means", "quats", "scales")], axis=0)
    by_comp = np.argsort(spread / (1.0 - d["comp"] ** 2), kind="stable")[:2]
    rest = [k for k in range(n_vis) if k not in by_comp][:3]
    only = {0: "v_depths"}
    if n_vis >= 5:
        only = dict(zip(rest, ("v_depths", "x_quat", "x_mean")))
        only.update({int(by_comp[0]): "v_comp", int(by_comp[1]): "v_opac_eff"})
    zero[list(only)] = False
    for key, v in rows.items():
        if key in ("x_abs", "x_col"):
            continue
        v[zero] = 0
        for row, keep in only.items():
            if keep != key:
                v[row] = 0
    rows = {k: v.astype(F) for k, v in rows.items()}
    return ids, rows, zero, d, only


def scatter(N, ids, v):
    """[1, N, .]: rows v at the places ids, zeros elsewhere."""
    out = np.zeros((1, N) + v.shape[1:], v.dtype)
    out[0, ids] = v
    return out


def compact_reference(rows, ids, d, aa=True, vcomp=True, voe=True, xq=True, xm=True, mags=None):
    """The reference of a compact call on the large scene: name -> (value, terms), dense [N, .]."""
    sc = scene(BIG)
    N = sc.N
    dense = {k: scatter(N, ids, np.asarray(v)) for k, v in rows.items()}
    V, M = cotangent_matrix(d, sc.opac, dense["v_means2d"], dense["v_depths"], dense["v_conics"], dense["v_comp"] if vcomp else None,
                            dense["v_opac_eff"] if voe else None, aa, mags=mags)
    return backward(1, N, d, V, M, sc.opac, dense["v_opac_eff"] if voe else None, aa, dense["x_quat"][0] if xq else None,
                    dense["x_mean"][0] if xm else None)


def ws_rows(ref, ids):
    """[n_vis, 12] value and terms of the workspace rows: v_mean 3 | v_quat 4 | v_scale 3 | v_opacity | pad."""
    out = []
    for j in (0, 1):
        opac = ref["opacities"][j] if "opacities" in ref else np.zeros(ref["means"][0].shape[0])
        out.append(np.concatenate([ref["means"][j][ids], ref["quats"][j][ids], ref["scales"][j][ids], opac[ids, None], np.zeros((ids.size, 1))], 1))
    return out


def blended_opacity(ids):
    """opacity x compensation of the large scene's Gaussians as front.hip forms it: one float32 product."""
    return (scene(BIG).opac[ids] * scene_forward(BIG)["comp32"][0, ids]).astype(F)


def row_gradients(G, ids, raw, depth_col=None, v_comp=None):
    """Gradient rows G [n_vis, >= 8] = [v_xy 2 | |v_xy| 2 | v_conic 3 | v_opacity_eff | ...] (raw: the raw moments of those) -> the rows
    and magnitudes compact_reference takes, and the converted first eight columns with their magnitudes."""
    n_vis = ids.size
    N = scene(BIG).N
    if raw:
        conv, mag = raw_to_gradients(G, scene_forward(BIG)["conics32"][0, ids], blended_opacity(ids))
    else:
        conv, mag = G[:, :8].astype(np.float64), np.abs(G[:, :8]).astype(np.float64)
    v_depth = np.zeros(n_vis) if depth_col is None else G[:, depth_col].astype(np.float64)
    rows = dict(v_means2d=conv[:, 0:2], v_conics=conv[:, 4:7], v_depths=v_depth, v_comp=np.zeros(n_vis, F) if v_comp is None else v_comp,
                v_opac_eff=G[:, 7], x_quat=np.zeros((n_vis, 4)), x_mean=np.zeros((n_vis, 3)))
    mags = dict(means2d=scatter(N, ids, mag[:, 0:2]), conics=scatter(N, ids, mag[:, 4:7]), depths=scatter(N, ids, np.abs(v_depth)))
    return rows, mags, conv, mag


def eighth_only_row(n_vis):
    """The raw row that is non-zero in its eighth float only (v_opacity_eff: the compensation's VJP alone, see compact_case); None with
    fewer than five rows, where it would be a camera gradient's only term."""
    _, _, _, _, only = compact_case(n_vis)
    return next((k for k, v in only.items() if v == "v_opac_eff"), None)


def gradient_rows(n_vis, raw):
    """[n_vis, 8] float32 = [v_xy 2 | |v_xy| 2 | v_conic 3 | v_opacity_eff] of compact_case's Gaussians from the scene's OWN cotangents
    (the ones the generator's sibling limit was applied with), or the raw moments that convert to them: with o the blended opacity,
    (m1, m2) = -conic^-1 v_xy / o, (m3, m4, m5) = -(2 v_a, v_b, 2 v_c) / o, rounded to float32."""
    ids, rows, _, _, _ = compact_case(n_vis)
    c = scene(BIG).cot
    G = np.zeros((n_vis, 8))
    G[:, 0:2], G[:, 4:7], G[:, 7] = c["v_means2d"][0, ids], c["v_conics"][0, ids], c["v_opac_eff"][0, ids]
    G[:, 2:4] = np.abs(G[:, 0:2]) * 1.5
    if raw:
        o = blended_opacity(ids).astype(np.float64)
        a, b, cc = (scene_forward(BIG)["conics32"][0, ids, k].astype(np.float64) for k in range(3))
        det = a * cc - b * b
        vx, vy = G[:, 0].copy(), G[:, 1].copy()
        G[:, 0], G[:, 1] = -(cc * vx - b * vy) / det / o, -(a * vy - b * vx) / det / o
        G[:, 2:4] *= B.HALF_LOG2E / o[:, None]
        G[:, 4], G[:, 5], G[:, 6] = -2 * G[:, 4] / o, -G[:, 5] / o, -2 * G[:, 6] / o
    return G


@functools.lru_cache(maxsize=None)
def raw_case(n_vis):
    """Raw-moment rows [n_vis, 12]: moments 0 .. 7 (gradient_rows) | colours 8 .. 10 | v_depth 11, for the Gaussians of compact_case:
    its zero rows, and row eighth_only_row(n_vis) non-zero in its eighth float only.  -> G float32, v_comp [n_vis] float32."""
    ids, _, zero, _, _ = compact_case(n_vis)
    c = scene(BIG).cot
    r = np.random.RandomState(77 + n_vis)
    G = np.concatenate([gradient_rows(n_vis, True), r.standard_normal((n_vis, 3)), c["v_depths"][0, ids, None]], axis=1)
    G[zero] = 0
    v_comp = np.where(zero, 0, c["v_comp"][0, ids]).astype(F)
    k = eighth_only_row(n_vis)
    if k is not None:
        G[k, :7], G[k, 8:], v_comp[k] = 0, 0, 0
    return G.astype(F), v_comp


def wire_cases():
    """(n_vis, D, with_depth, color_mode, raw_rows): every D with and without depth, then every colour mode with both row forms."""
    out = []
    for i, (D, depth) in enumerate((D, depth) for D in (0, 3, 4, 7) for depth in (0, 1)):
        out.append((NVIS[i % 5], D, depth, (0, 1, 2)[i % 3] if D >= 3 else 0, i % 2))
    return out + [(513, 3, 1, 1, 1), (257, 3, 0, 2, 1), (256, 4, 1, 1, 0), (255, 7, 0, 2, 0), (1, 7, 1, 0, 1), (513, 4, 0, 2, 1), (257, 7, 1, 1, 0)]


def wire_rows(n_vis, D, depth, raw):
    """Rows for mtgs_project_bwd_rows, four floats wider than 8 + D + depth rounded up to a multiple of 4: gradient_rows, random
    colours, the scene's depth cotangent; compact_case's zero rows, and row 1 non-zero in the last spare column only.
    -> G float32 [n_vis, stride], a generator for the colour inputs."""
    ids, _, zero, _, _ = compact_case(n_vis)
    stride = (8 + D + depth + 3) // 4 * 4 + 4
    r = np.random.RandomState(31 * n_vis + 7 * D + depth)
    G = r.standard_normal((n_vis, stride))
    G[:, :8] = gradient_rows(n_vis, raw)
    if depth:
        G[:, 8 + D] = scene(BIG).cot["v_depths"][0, ids]
    G[zero] = 0
    if n_vis > 1:
        G[1] = 0
        G[1, stride - 1] = 1.5
    return G.astype(F), r


# ---- comp == 0: flat Gaussians ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flat_case(oracle_forward):
    """Gaussians with two zero scales in front of the large scene's camera: the 2-D covariance before the blur has rank one, its
    determinant c00 c11 - c01^2 is a rounding residue of either sign, and wherever it is <= 0 the compensation is exactly 0.  That is
    where add_blur_vjp's division by comp + 1e-6 decides the result and autograd's sqrt has no derivative: the reference is gsplat's
    formula with the GIVEN compensation (derivatives(comp_in=...)), and the comparison that counts is with the C oracle.
    oracle_forward: oracle.project_fwd (float32; its conics and compensations are what a backward call is given).
    -> arrays (means, quats, scales, opac, viewmats, Ks), the oracle's forward, mask [1, n] (visible and comp == 0), cotangents, reference."""
    sc = scene(BIG)
    r = np.random.RandomState(21)
    pick = np.flatnonzero(sc.group < 0)[:96]
    n = pick.size
    scales = np.zeros((n, 3), F)
    scales[np.arange(n), r.randint(0, 3, n)] = r.uniform(0.05, 0.3, n)
    arrays = (sc.means[pick], sc.quats[pick], scales, sc.opac[pick], sc.viewmats, sc.Ks)
    fwd = oracle_forward(arrays[0], arrays[1], arrays[2], arrays[4], arrays[5], W, H, eps2d=EPS2D, near=NEAR, far=FAR, calc_compensations=True)
    mask = (fwd[0] > 0) & (fwd[4] == 0)
    cot = _cotangents(1, n, 2021)
    pc, pn = np.nonzero(mask)
    d = derivatives(arrays[0], arrays[1], arrays[2], arrays[4], arrays[5], pc, pn, comp_in=np.zeros(pc.size))
    d["comp"] = np.zeros(pc.size)                                       # (the given one: v_opacities = v_opac_eff x 0)
    V, M = cotangent_matrix(d, arrays[3], cot["v_means2d"], cot["v_depths"], cot["v_conics"], cot["v_comp"], cot["v_opac_eff"], True)
    # Terms of the compensation's part, one level below the components: the formula's two addends cancel entry by entry here (along the
    # Gaussian's one extended axis exactly), so the scale of its rounding is  |v| 0.5 / (comp + 1e-6) x
    # sum over the covariance's entries of (|1 - comp^2| |conic entry| + eps2d det(conic) on the diagonal) |d entry / d parameter|
    f = M[:, 6] * 0.5 / COMP_EPS
    M[:, 6] = 0
    ref = {k: list(v) for k, v in backward(1, n, d, V, M, arrays[3], cot["v_opac_eff"], True).items()}
    a, b, c = d["conics"].T
    w = np.stack([np.abs(a) + EPS2D * (a * c - b * b), 2 * np.abs(b), np.abs(c) + EPS2D * (a * c - b * b)], axis=1) * f[:, None]
    for name, idx in (("means", pn), ("quats", pn), ("scales", pn), ("viewmat", pc)):
        D = np.abs(d["cov"][name])
        np.add.at(ref[name][1], idx, (w[(slice(None), slice(None)) + (None,) * (D.ndim - 2)] * D).sum(axis=1))
    return arrays, fwd, mask, cot, {k: tuple(v) for k, v in ref.items()}


def oracle_flat(oracle):
    """The C oracle's backward on flat_case, v_opac_eff folded by the caller: name -> array."""
    a, fwd, mask, cot, _ = flat_case(oracle.project_fwd)
    v_comp = (cot["v_comp"] + cot["v_opac_eff"] * a[3][None]).astype(F)
    vm_, vq, vs, vvm = oracle.project_bwd(a[0], a[1], a[2], a[4], a[5], W, H, EPS2D, mask.astype(np.int32), fwd[3], fwd[4],
                                          cot["v_means2d"], cot["v_depths"], cot["v_conics"], v_comp)
    return dict(means=vm_, quats=vq, scales=vs, viewmat=vvm, opacities=(cot["v_opac_eff"] * fwd[4] * mask).sum(0))


def device_bound(measured):
    return B.device_bound(measured)


worst_ratio = B.worst_ratio

# The fp32 C oracle's worst |oracle - reference| / (2^-24 sum |terms|) over every scene, mask and option set of
# tests/test_project_refs_host.py::test_oracle_backward_within_constants and ::test_oracle_forward -- MEASURED there, against the oracle
# (fp32, contraction off, v_opac_eff folded by the caller as tests/test_oracle_vs_torch_ref.py::oracle_backward does) and never against
# a HIP kernel; the tests assert that the oracle stays within them.  The rows of the compact path and the wire rows (compact_case,
# raw_case, wire_rows; ::test_oracle_on_the_compact_inputs) are part of the maximum.  Rounded up.
ORACLE_BWD = {"means": 24.7, "quats": 156.0, "scales": 147.0, "opacities": 2.8, "viewmat": 6.2}
# The flat Gaussians of flat_case alone (comp == 0), measured by ::test_oracle_flat_gaussians: the compensation's cotangent is
# multiplied by 0.5 / 1e-6 there and conic - eps2d det(conic) has one eigenvalue that cancels exactly, so the compensation's terms are
# taken one level below the components (flat_case; with the component-level terms the oracle itself measures 6e9).  The device is
# compared with the ORACLE on them: |device - oracle| <= |device - reference| +
# |oracle - reference| <= (device_bound(constant) + constant) x 2^-24 terms.
ORACLE_BWD_FLAT = {"means": 9.8, "quats": 6.5, "scales": 3.3, "opacities": 0.0, "viewmat": 0.9}
ORACLE_FWD = {"means2d": 2.9, "depths": 1.9, "conics": 10.8, "comp": 3.4}
