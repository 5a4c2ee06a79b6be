"""Plain float64 references, input builders and case tables of the visible-row colour kernels (csrc/viscolor.hip, wild.hip,
normals.hip), shared by tests/test_gpu_row_colors.py (the device against them) and tests/test_row_refs_host.py (the references
against independent formulations, and the conditioning of every case, without a GPU).  TEST INFRASTRUCTURE ONLY; nothing under
mtgs_amd/ imports this.

Conventions
  * inputs are the float32 CPU tensors the device call receives; where the kernel forms an argument in float32 (dc + dc_add, the
    clamp's pre-activation that decides the pass-through mask) the reference forms the same float32 number first;
  * a case is well-conditioned when float32 and float64 must take the same decision everywhere (clamp side, ReLU side, normal
    flip, smallest scale): the builders return the margins, the host test asserts them for every case of the tables below, and
    the GPU test then compares masks and zero patterns for identity -- no row is left out of any comparison.
"""
import numpy as np
import torch

from oracle import normals_oracle as no
from oracle.torch_ref import sh_bases

U32 = 2.0 ** -24          # unit roundoff of float32
C0 = 0.28209479177387814
REC = 16                  # floats of a packed record (csrc/raster_rec.hpp); channels start at float 8
POISON_BITS = 0x7FC5A5A5  # a quiet NaN with a recognisable payload: "must not be read" / "must be overwritten or left alone"
FLUSH = 4.8e-38           # colour cotangents below this count as zero (viscolor.hip)


# ---- small plumbing -------------------------------------------------------------------------------------------------------------
def totals_word(n, dev="cpu"):
    """The device row count as the kernels read it: the int64 n << 32 (low half: the front end's other counter, arbitrary)."""
    return torch.tensor([(int(n) << 32) | 0x1234], dtype=torch.int64, device=dev)


def poisoned(shape, dev="cpu"):
    return torch.full(shape, POISON_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def bits(t):
    """The bit patterns of a float32 tensor (comparisons that also hold for NaN and -0.0)."""
    return t.detach().contiguous().cpu().view(torch.int32)


def is_poison(t):
    return bits(t) == POISON_BITS


def sorted_subset(N, n, seed, must=()):
    """n sorted distinct Gaussian indices out of N (int32), holding every index of `must`."""
    g = torch.Generator().manual_seed(seed)
    must = sorted(set(int(m) for m in must))
    assert len(must) <= n <= N
    rest = [i for i in torch.randperm(N, generator=g).tolist() if i not in set(must)][:n - len(must)]
    return torch.tensor(sorted(must + rest), dtype=torch.int32)


def padded_ids(vis, N, alloc):
    """vis_ids of `alloc` rows: `vis`, then in-range indices of OTHER Gaussians (every index a kernel could meet is valid; the
    rows past the count must still not be touched, which the tests see on those Gaussians and rows)."""
    used = set(vis.tolist())
    others = [i for i in range(N) if i not in used]
    tail = [others[i % len(others)] if others else 0 for i in range(alloc - len(vis))]
    return torch.cat([vis, torch.tensor(tail, dtype=torch.int32)])


def grad_rows(cot, alloc, RS, col, seed=0):
    """Compact gradient rows G [alloc, RS]: the cotangent in columns col .. col + 2, seeded noise in every other column."""
    g = torch.Generator().manual_seed(1000 + seed)
    G = torch.randn(alloc, RS, generator=g)
    G[:cot.shape[0], col:col + 3] = cot
    return G


def edge_dc():
    """features_dc values whose fp32 dc * C0 + 0.5 is exactly 0 or exactly 1 (the clamp's edges), and their neighbours."""
    c0 = np.float32(C0)
    out = []
    for target in (0.0, 1.0):
        d = np.float32((target - 0.5) / C0)
        for _ in range(64):
            x = np.float32(np.float32(d * c0) + np.float32(0.5))
            if x == target:
                break
            d = np.nextafter(d, np.float32(np.inf) if x < target else np.float32(-np.inf), dtype=np.float32)
        assert np.float32(np.float32(d * c0) + np.float32(0.5)) == target
        out += [d, np.nextafter(d, np.float32(np.inf), dtype=np.float32), np.nextafter(d, np.float32(-np.inf), dtype=np.float32)]
    return torch.tensor(np.array(out, dtype=np.float32))


# ---- appearance MLP (moved from tests/test_gpu_wild.py, which imports them back) ------------------------------------------------
def wild_params(N, seed=0, with_emb=True, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    dc = (torch.rand(N, 3, generator=g) - 0.5) * 1.2 / C0      # about a fifth of the channels beyond the clamp
    if N >= 6:
        e = edge_dc()
        dc.view(-1)[:e.numel()] = e[:min(e.numel(), 3 * N)]
    rest = 0.3 * torch.randn(N, 15, 3, generator=g)
    emb = torch.randn(32, generator=g) if with_emb else None
    mlp = torch.nn.Sequential(torch.nn.Linear(59, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(),
                              torch.nn.Linear(128, 6))
    torch.manual_seed(seed)
    for m in mlp:
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.uniform_(m.weight, -0.15, 0.15)
            torch.nn.init.uniform_(m.bias, -0.1, 0.1)
    with torch.no_grad():        # (so that the network's output is not lost under the 0.01)
        mlp[4].weight.mul_(20.0)
        mlp[4].bias.mul_(20.0)
    ts = [dc, rest, emb, mlp[0].weight.detach(), mlp[0].bias.detach(), mlp[2].weight.detach(), mlp[2].bias.detach(),
          mlp[4].weight.detach(), mlp[4].bias.detach()]
    return [None if t is None else t.clone().to(dev).requires_grad_(True) for t in ts]


def wild_reference(ts, kinks=None):
    """float64 evaluation of the formula; the clamp's pass-through mask is taken from the fp32 pre-activation (inclusive edges,
    as torch.clamp), which is what the fp32 kernel sees.  kinks (a list): receives the rows with a hidden pre-activation within
    1e-5 of zero, where fp32 and float64 may take different sides of a ReLU."""
    dc, rest, emb, w1, b1, w2, b2, w3, b3 = ts
    N = dc.shape[0]
    pre32 = (dc.detach() * torch.tensor(C0, dtype=torch.float32)) + 0.5
    mask = (pre32 >= 0) & (pre32 <= 1)
    pre = dc.double() * C0 + 0.5
    rgb = torch.where(mask, pre, pre32.clamp(0, 1).double())
    e = torch.zeros(32, dtype=torch.float64, device=dc.device) if emb is None else emb.double().reshape(32)
    x = torch.cat([rgb, rest.double().reshape(N, 45)[:, :24], e.expand(N, 32)], dim=1)
    z1 = x @ w1.double().T + b1.double()
    h = torch.relu(z1)
    z2 = h @ w2.double().T + b2.double()
    h = torch.relu(z2)
    if kinks is not None:
        kinks.append(((z1.detach().abs() < 1e-5).any(1) | (z2.detach().abs() < 1e-5).any(1)))
    y = 0.01 * (h @ w3.double().T + b3.double())
    return rgb * (1 + y[:, 3:6]) + y[:, :3]


WILD_ROWS = [0, 1, 31, 32, 33, 64, 65, 8191, 8192, 8193, 8225]     # 32-row tile; WILD_GRID * WT = 8192: the first grid-strided tile
WILD_N = 515 * 32                                                  # > 2 * 8225 + 1: the visible rows are the odd Gaussians 1, 3, 5, ...
WILD_GRAD_ROWS = [1, 33, 65, 8193]                                 # the weight-gradient cases (a reference backward each)
WILD_NAMES = ("features_dc", "features_rest", "embedding", "w1", "b1", "w2", "b2", "w3", "b3")
_wild_cache = {}


def wild_case(with_emb):
    """The one parameter set of every appearance-MLP case (CPU, float32): WILD_N Gaussians, the edge dc values in rows 0 and 1
    (Gaussian 1 is the first visible row), a cotangent [WILD_N, 3] that is ZERO on the rows at a ReLU kink (a hidden
    pre-activation within 1e-5 of zero: there fp32 and float64 may take different sides), and that kink mask."""
    if with_emb not in _wild_cache:
        ts = [None if t is None else t.detach() for t in wild_params(WILD_N, seed=21, with_emb=with_emb, dev="cpu")]
        cot = torch.randn(WILD_N, 3, generator=torch.Generator().manual_seed(22))
        kinks = []
        with torch.no_grad():
            wild_reference(ts, kinks)
        cot[kinks[0]] = 0.0
        _wild_cache[with_emb] = (ts, cot, kinks[0])
    return _wild_cache[with_emb]


def wild_vis_ids(rows):
    return (torch.arange(rows, dtype=torch.int32) * 2 + 1)


def wild_backward_ref(ts, cot, dtype=torch.float64):
    """Gradients of sum(colour * cot) for the nine inputs by plain formulas in `dtype` (float64: the reference; float32: the
    measurement behind C_WILD), and, per weight-gradient element, sum |term| of the sum over rows that forms it.  The clamp
    mask comes from the float32 pre-activation in both."""
    dc, rest, emb, w1, b1, w2, b2, w3, b3 = [None if t is None else t.detach() for t in ts]
    N = dc.shape[0]
    f = lambda t: t.to(dtype)
    pre32 = dc * torch.tensor(C0, dtype=torch.float32) + 0.5
    mask = ((pre32 >= 0) & (pre32 <= 1)).to(dtype)
    rgb = pre32.clamp(0, 1).to(dtype) if dtype == torch.float32 else torch.where(mask > 0, f(dc) * C0 + 0.5, pre32.clamp(0, 1).double())
    e = torch.zeros(32, dtype=dtype) if emb is None else f(emb).reshape(32)
    x = torch.cat([rgb, f(rest).reshape(N, 45)[:, :24]], 1)
    b1e = f(b1) + f(w1)[:, 27:] @ e
    h1 = torch.relu(x @ f(w1)[:, :27].T + b1e)
    h2 = torch.relu(h1 @ f(w2).T + f(b2))
    y = 0.01 * (h2 @ f(w3).T + f(b3))
    g = f(cot)
    dz = 0.01 * torch.cat([g, g * rgb], 1)
    dh2 = (dz @ f(w3)) * (h2 > 0)
    dh1 = (dh2 @ f(w2)) * (h1 > 0)
    dx = dh1 @ f(w1)[:, :27]
    s1 = dh1.sum(0)
    grads = {"features_dc": mask * (g * (1 + y[:, 3:6]) + dx[:, :3]) * C0,
             "features_rest": torch.cat([dx[:, 3:], torch.zeros(N, 21, dtype=dtype)], 1).reshape(N, 15, 3),
             "w1": torch.cat([dh1.T @ x, s1[:, None] * e[None, :]], 1), "b1": s1, "w2": dh2.T @ h1, "b2": dh2.sum(0),
             "w3": dz.T @ h2, "b3": dz.sum(0), "embedding": f(w1)[:, 27:].T @ s1}
    # sum |term| with every factor expanded down to the inputs (the running bound of a float32 evaluation: a hidden activation
    # or a back-propagated factor is itself a float32 dot product with cancellation, whose error is relative to the sum of the
    # absolute products behind it, not to its value)
    w1a, w2a, w3a = f(w1).abs(), f(w2).abs(), f(w3).abs()
    H1 = (x.abs() @ w1a[:, :27].T + f(b1).abs() + w1a[:, 27:] @ e.abs()) * (h1 > 0)
    H2 = (H1 @ w2a.T + f(b2).abs()) * (h2 > 0)
    D2 = (dz.abs() @ w3a) * (h2 > 0)
    D1 = (D2 @ w2a) * (h1 > 0)
    a1 = D1.sum(0)
    terms = {"w1": torch.cat([D1.T @ x.abs(), a1[:, None] * e.abs()[None, :]], 1), "b1": a1, "w2": D2.T @ H1, "b2": D2.sum(0),
             "w3": dz.abs().T @ H2, "b3": dz.abs().sum(0), "embedding": w1a[:, 27:].T @ a1}
    return grads, terms


# |weight gradient (float32) - float64| <= C_WILD 2^-24 sum |term| per element, the terms being the products behind the element
# expanded down to the inputs (wild_backward_ref).  Measured on the CPU: the whole backward in float32 (torch matmuls, rows in
# order) against float64 over WILD_GRAD_ROWS with and without the embedding: worst ratio 2.47 (w2, one row, no embedding; 1.86 with
# the embedding, 1.42 at 33 rows, 1.25 for w1, below 1 for w3, the biases and the embedding).  Times 4 for the device's order (MFMA k-steps, 32-row
# tiles, per-workgroup partials) and FMA contraction.  tests/test_row_refs_host.py asserts that the float32 evaluation stays
# within a quarter of the bound.  What the constant rests on: torch float32 on the CPU (not a transcription of the MFMA order) and
# the expanded sum |term| above, which is wider than the products of an element's own factors; nothing was measured on a device.
C_WILD = 10.0


# ---- spherical-harmonics colour rows --------------------------------------------------------------------------------------------
def sh_poly(xyz):
    """The 16 real SH basis polynomials of degree <= 3 at an UNNORMALISED point [n, 3] -> [n, 16] (gsplat's constants; equal to
    oracle/torch_ref.py::sh_bases on the unit sphere): the extension the kernel differentiates before it projects."""
    x, y, z = xyz.unbind(-1)
    z2, c1, s1 = z * z, x * x - y * y, 2 * x * y
    t0b, t0c, t1b = -1.092548430592079 * z, -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
    return torch.stack([torch.full_like(x, 0.2820947917738781), -0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x,
                        0.5462742152960395 * s1, t0b * y, 0.9461746957575601 * z2 - 0.3153915652525201, t0b * x, 0.5462742152960395 * c1,
                        -0.5900435899266435 * (x * s1 + y * c1), t1b * s1, t0c * y, z * (1.865881662950577 * z2 - 1.119528997770346),
                        t0c * x, t1b * c1, -0.5900435899266435 * (x * c1 - y * s1)], -1)


def sh_rows_ref(degree, dirs_raw, dc, add, rest, k_rest, use_sh, cot=None, exact=None, dtype=torch.float64):
    """One colour row per Gaussian, all rows of the inputs.  dirs_raw [n,3] (normalised inside), dc [n,3], add [n,3] or None,
    rest [n,15,3], k_rest / use_sh int64 [n] (the node's fields per Gaussian), exact bool [n]: rows whose SH sum is the single
    product C0 dc (no other active coefficient): their float32 pre-activation is formed exactly as the kernel forms it.
    use_sh 0: sigmoid(dc sum); 1: clamp(. + 0.5, 0, 1); 4: clamp_min(. + 0.5, 0).
    Returns a dict: colour [n,3], mask (uint8 bits, 7 for the sigmoid), pre (the float64 pre-activation), and with cot [n,3]:
    feat [n,16,3] (d L / d coefficient k; dc and dc_add share column 0), feat_autograd (the same through autograd), ddir [n,3]
    (through normalize, autograd), dterms [n,3] (sum |term| of the direction gradient of the row, for the dir_part bound)."""
    n = dirs_raw.shape[0]
    NB = (degree + 1) ** 2
    k_rest, use_sh = torch.as_tensor(k_rest).long().reshape(n), torch.as_tensor(use_sh).long().reshape(n)
    c0 = dc if add is None else dc + add                       # (float32, as lane 0 adds them)
    cfull = torch.cat([c0.reshape(n, 1, 3), rest.reshape(n, 15, 3)], 1).to(dtype).requires_grad_(True)
    d = dirs_raw.to(dtype).clone().requires_grad_(True)
    kk = torch.arange(16)
    act = ((kk[None] < NB) & (kk[None] - 1 < k_rest[:, None])).to(dtype)
    sig = use_sh == 0
    B = torch.zeros(n, 16, dtype=dtype)
    B[:, :NB] = sh_bases(degree, d) if n else B[:, :NB]
    B = torch.where(sig[:, None], (kk[None] == 0).to(dtype).expand(n, 16), B * act)
    s = (B[:, :, None] * cfull).sum(1)
    pre = s + 0.5
    pre32 = pre.detach().float()
    if exact is not None and bool(exact.any()):
        ex32 = c0 * torch.tensor(0.2820947917738781, dtype=torch.float32) + 0.5      # two roundings, as the kernel's
        pre32 = torch.where(exact[:, None], ex32, pre32)
    lo, hi = pre32 >= 0, pre32 <= 1
    m3 = torch.where(sig[:, None], torch.ones_like(lo), torch.where((use_sh == 4)[:, None], lo, lo & hi))
    clamped = torch.where((use_sh == 4)[:, None], pre32.clamp_min(0), pre32.clamp(0, 1)).to(dtype)
    colour = torch.where(sig[:, None], torch.sigmoid(s), torch.where(m3, pre, clamped))
    out = {"colour": colour.detach(), "pre": pre.detach(), "pre32": pre32,
           "mask": (m3[:, 0].int() | (m3[:, 1].int() << 1) | (m3[:, 2].int() << 2)).to(torch.uint8)}
    if cot is None:
        return out
    v = torch.where(cot.abs() < FLUSH, torch.zeros_like(cot), cot).to(dtype)
    if n:
        (colour * v).sum().backward()
    out["feat_autograd"] = torch.zeros(n, 16, 3, dtype=dtype) if cfull.grad is None else cfull.grad
    out["ddir"] = torch.zeros(n, 3, dtype=dtype) if d.grad is None else d.grad
    dact = torch.where(sig[:, None], (colour * (1 - colour)).detach(), m3.to(dtype))
    out["feat"] = B.detach()[:, :, None] * (dact * v)[:, None, :]
    # sum |term| of the direction gradient: lane k contributes w_k grad b_k (w_k = <coefficient k, masked cotangent>), the row
    # sums them, projects off the direction (g - n <n, g>) and divides by the length
    with torch.enable_grad():
        u = (d.detach() / d.detach().norm(dim=-1, keepdim=True)).requires_grad_(True)
        P = sh_poly(u)
        J = torch.stack([torch.autograd.grad(P[:, k].sum(), u, retain_graph=True)[0] for k in range(16)], 1) if n else torch.zeros(0, 16, 3, dtype=dtype)
    w = (cfull.detach() * (m3.to(dtype) * cot.to(dtype))[:, None, :]).sum(-1) * act * (~sig[:, None]) * (kk[None] > 0)
    T = (w.abs()[:, :, None] * J.abs()).sum(1)
    un = u.detach().abs()
    out["dterms"] = (T + un * (un * T).sum(-1, keepdim=True)) / d.detach().norm(dim=-1, keepdim=True)
    out["dir_w"], out["dir_J"], out["dir_u"], out["dir_len"] = w, J, u.detach(), d.detach().norm(dim=-1, keepdim=True)
    return out


# |dir_part (float32) - float64| <= C_DIR 2^-24 sum over the workgroup's rows of dterms, per component.  Measured on the CPU:
# the direction gradient of every SH case below in float32 (torch, the kernel's formula: lane products, row sum, projection,
# division by the length, rows added in order) against float64: worst ratio 2.68.  Times 4 for the device's order (a 16-lane
# tree per row, a wave tree and four waves per workgroup) and FMA contraction.  Rests on torch float32 on the CPU with the
# lane weights w_k taken from float64; nothing was measured on a device.
C_DIR = 11.0


def dir_rows_f32(r):
    """The direction gradient of sh_rows_ref's rows by the kernel's formula in float32 (the measurement behind C_DIR)."""
    w, J, u, ln = r["dir_w"].float(), r["dir_J"].float(), r["dir_u"].float(), r["dir_len"].float()
    g = (w[:, :, None] * J).sum(1)
    return (g - u * (g * u).sum(-1, keepdim=True)) / ln


# One SH case: (name, n_rows, cap_extra, totals_extra, degree, k_rest, use_sh, add, strided, n_nodes).  n = min(n_rows +
# totals_extra, cap) rows are written, cap = n_rows + cap_extra; use_sh / k_rest alternate between the nodes where the case has two.
def _sh_cases():
    cases = []
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 129):
        cases.append((f"n{n}", n, 0, 0, 3, 15, 1, False, False, 2))
    for n, extra in ((17, 1), (64, 70), (65, 1), (129, 70), (0, 70)):
        cases.append((f"n{n}_cap+{extra}", n, extra, 0, 3, 15, 1, True, False, 2))
    cases.append(("totals>cap", 65, 0, 5, 3, 15, 1, False, False, 2))
    i = 0
    for degree in range(4):
        for k_rest in (0, 3, 8, 15):
            cases.append((f"deg{degree}_k{k_rest}", 65, 0, 0, degree, k_rest, (0, 1, 4)[i % 3], i % 2 == 1, (i // 2) % 2 == 1, 1 + i % 2))
            i += 1
    for use_sh in (0, 1, 4):
        for add in (False, True):
            cases.append((f"use{use_sh}_add{int(add)}", 33, 3, 0, 2, 8, use_sh, add, True, 2))
    return cases


SH_CASES = _sh_cases()
SH_SEEDS = {}             # replacement seeds of the cases whose first draw is not well-conditioned (test_row_refs_host.py)
SH_N = 300                # Gaussians of an SH scene (the visible rows are a subset)
RS, COL = 16, 8           # gradient-row stride and the colour columns, as the rasterization's compaction rows


def sh_scene(name, n_rows, degree, k_rest, use_sh, add, n_nodes, N=SH_N, edge_rows=False, nodes=None, must=None):
    """Deterministic inputs of an SH case (CPU, float32): coefficients, means, camera, vis_ids (n_rows sorted indices holding the
    first and last Gaussian of every node), the cotangent (rows 2 mod 5 zero, rows 3 mod 10 below the flush threshold), the node
    split [(start, n, k_rest, use_sh)] and the per-Gaussian node fields."""
    seed = SH_SEEDS.get(name, 0) * 7919 + sum(ord(c) * (i + 1) for i, c in enumerate(name))
    g = torch.Generator().manual_seed(seed)
    dc = torch.randn(N, 3, generator=g) * 1.2
    addt = torch.randn(N, 3, generator=g) * 0.3 if add else None
    rest = torch.randn(N, 15, 3, generator=g) * 0.25
    means = torch.randn(N, 3, generator=g) * 4
    cam = torch.tensor([0.3, -0.2, 9.0])
    if nodes is not None:
        pass
    elif n_nodes == 1:
        nodes = [(0, N, k_rest, use_sh)]
    else:
        cut = 131
        nodes = [(0, cut, k_rest, use_sh), (cut, N - cut, 15 if k_rest == 15 else max(k_rest - 1, 0), use_sh)]
    kr = torch.cat([torch.full((n,), k) for _, n, k, _ in nodes]).long()
    us = torch.cat([torch.full((n,), u) for _, n, _, u in nodes]).long()
    if must is None:
        must = [i for s, n, _, _ in nodes if n for i in (s, s + n - 1)]
    must = sorted(set(must))[:n_rows]
    vis = sorted_subset(N, n_rows, seed + 1, must)
    cot = torch.randn(n_rows, 3, generator=g)
    idx = torch.arange(n_rows)
    cot[idx % 5 == 2] = 0.0
    cot[idx % 10 == 3] = 1e-38
    exact = torch.zeros(N, dtype=torch.bool)
    if edge_rows:       # the clamp's edges and their float32 neighbours on the dc term alone: every other coefficient is zero
        e = edge_dc()
        rows = vis[:6].long()
        rest[rows] = 0.0
        dc[rows] = torch.randn(6, 3, generator=g)
        dc[rows, 0] = e
        dc[rows[:3], 1] = e[3:]
        above, c0 = np.float32(e[3]), np.float32(0.2820947917738781)      # the first dc whose pre-activation is ABOVE 1 (the next
        while np.float32(np.float32(above * c0) + np.float32(0.5)) <= 1:     # float32 after the edge value may still round to 1)
            above = np.nextafter(above, np.float32(np.inf), dtype=np.float32)
        dc[rows[0], 2] = float(above)
        if addt is not None:
            addt[rows] = 0.0
        exact[rows] = True
        cot[:6] = torch.randn(6, 3, generator=g)
    return {"dc": dc, "add": addt, "rest": rest, "means": means, "cam": cam, "vis": vis, "cot": cot, "nodes": nodes, "k_rest": kr,
            "use_sh": us, "exact": exact, "N": N, "degree": degree}


TABLE_FIELDS = [(15, 1), (8, 4), (3, 1), (0, 0), (15, 4)]      # (k_rest, use_sh) of node i mod 5: a wrong node is a wrong colour


def sh_table_scene():
    """One scene under two tables: 129 nodes (read from global memory) and the same with one EMPTY middle node dropped, 128 (the
    LDS table), so that every Gaussian keeps its node fields.  The visible rows hold the first and the last Gaussian of every
    third non-empty node, among them Gaussians whose `start` is shared with empty nodes in front of theirs."""
    split = split_nodes(SH_N, 129, 4)
    nodes129 = [(s, n) + TABLE_FIELDS[i % 5] for i, (s, n) in enumerate(split)]
    drop = 129 // 2
    assert nodes129[drop][1] == 0
    nodes128 = nodes129[:drop] + nodes129[drop + 1:]
    full = [(s, n) for s, n, _, _ in nodes129 if n]
    must = [i for s, n in full[::3] for i in (s, s + n - 1)] + [nodes129[drop + 2][0], nodes129[10][0]]
    sc = sh_scene("tables", 129, 3, 15, 1, True, 129, nodes=nodes129, must=must)
    sc["nodes128"] = nodes128
    return sc


OPT_USE_SH = [0, 1, 4]
TWIN_CASES = [(1, 16), (4, 16), (4, 9), (4, 4), (4, 1)]      # (use_sh, K): degree 3, 2, 1, 0 for K = 16, 9, 4, 1


def sh_opts_scene(use_sh):
    """The scene of the option test (coef_rows, row_flags, dirs, zero cotangents): two nodes with dc_add."""
    return sh_scene("opts", 70, 3, 15, use_sh, True, 2)


def sh_twin_scene(use_sh, K):
    """[N, K, 3] coefficient tensors as the public constructors take them: two K = 16 nodes (use_sh 1) or one node (use_sh 4)."""
    return sh_scene("twin", 70, {16: 3, 9: 2, 4: 1, 1: 0}[K], K - 1, use_sh, False, 2 if use_sh == 1 else 1)


def sh_edge_scene(use_sh):
    return sh_scene("edges", 33, 3, 15, use_sh, True, 1, edge_rows=True)


def sh_scene_ref(sc, dirs=None):
    """sh_rows_ref of a scene's VISIBLE rows, in row order."""
    v = sc["vis"].long()
    d = (sc["means"] - sc["cam"])[v] if dirs is None else dirs[v]
    return sh_rows_ref(sc["degree"], d, sc["dc"][v], None if sc["add"] is None else sc["add"][v], sc["rest"][v], sc["k_rest"][v],
                       sc["use_sh"][v], sc["cot"], sc["exact"][v])


def sh_margins(sc, ref):
    """The distance of every non-deliberate clamp pre-activation of the visible rows from the clamp's edges (use_sh 1: 0 and 1;
    4: 0), smallest first: inf when there is none."""
    v = sc["vis"].long()
    us, ex = sc["use_sh"][v], sc["exact"][v]
    pre = ref["pre"]
    m = torch.full_like(pre, float("inf"))
    m = torch.where((us == 1)[:, None], torch.minimum(pre.abs(), (pre - 1).abs()), m)
    m = torch.where((us == 4)[:, None], pre.abs(), m)
    m = torch.where(ex[:, None], torch.full_like(m, float("inf")), m)
    return float(m.min()) if m.numel() else float("inf")


def split_nodes(N, n_nodes, seed):
    """N Gaussians split into n_nodes nodes of mostly 1 to 3 Gaussians, with empty nodes in front, in the middle and behind (the
    last non-empty node takes what is left).  Returns [(start, n)]."""
    g = torch.Generator().manual_seed(seed)
    if n_nodes == 1:
        return [(0, N)]
    if n_nodes == 2:
        return [(0, N // 3), (N // 3, N - N // 3)]
    sizes = (torch.randint(1, 4, (n_nodes,), generator=g)).tolist()
    for i in (0, 1, n_nodes // 2, n_nodes // 2 + 1, n_nodes - 1, n_nodes - 2, 7, 8, 9):
        sizes[i] = 0
    last = max(i for i in range(n_nodes) if sizes[i])
    sizes[last] = 0
    assert sum(sizes) < N
    sizes[last] = N - sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return [(int(s), int(n)) for s, n in zip(starts, sizes)]


def node_table(nodes, dcS, addS, restS, dev):
    """A raw mtgs_node_desc table over ONE storage tensor per coefficient kind (dcS [N, dc_stride], addS [N, add_stride] or None,
    restS [N, rest_stride], device float32): node i is the rows [start, start + n) of them.  nodes: [(start, n, k_rest, use_sh)].
    For what the public constructors cannot express (k_rest / strides per node, dc_add, 129 nodes, empty nodes)."""
    from mtgs_amd import nodes as nd
    tab = np.zeros(len(nodes), dtype=nd._DESC)
    fb = 0
    for i, (s, n, k, u) in enumerate(nodes):
        tab["n"][i], tab["start"][i], tab["first_block"][i] = n, s, fb
        fb += -(-n // 256)
        tab["features_dc"][i] = dcS.data_ptr() + 4 * s * dcS.stride(0)
        tab["features_rest"][i] = restS.data_ptr() + 4 * s * restS.stride(0)
        tab["dc_stride"][i], tab["rest_stride"][i], tab["dc_add_stride"][i] = dcS.stride(0), restS.stride(0), 3
        if addS is not None:
            tab["features_dc_add"][i], tab["dc_add_stride"][i] = addS.data_ptr() + 4 * s * addS.stride(0), addS.stride(0)
        tab["k_rest"][i], tab["use_sh"][i] = k, u
    return nd._upload(tab, dev)


# ---- rows_expand ----------------------------------------------------------------------------------------------------------------
# (N, width, row_stride): 48-wide aligned rows at 1023 / 1024 / 1025 float4s per launch quantum (N * 12 float4s does not hit them:
# widths 4 and 12 do), the element-wise kernel through width 45 and through an odd row stride, and N = 0
EXPAND_CASES = [(0, 48, 48), (1, 48, 48), (85, 48, 48), (86, 48, 52), (1023, 4, 4), (1024, 4, 8), (1025, 4, 4), (341, 12, 12),
                (342, 12, 12), (23, 45, 48), (1023, 45, 45), (64, 48, 49), (1025, 3, 5)]


# ---- normals --------------------------------------------------------------------------------------------------------------------
NORMAL_ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 513]


def normals_scene(rows, seed=None):
    """N = 2 rows + 5 Gaussians (CPU float32), the visible rows a sorted subset; every mean is moved along the view ray's
    perpendicular until |dot(n0, view)| >= 1e-3 holds with room (0.05), so no flip is near its threshold."""
    N = 2 * rows + 5
    g = torch.Generator().manual_seed(rows * 13 + 5 if seed is None else seed)
    quats = torch.randn(N, 4, generator=g)
    scales = torch.exp(torch.randn(N, 3, generator=g))
    means = torch.randn(N, 3, generator=g) * 10
    A = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
    c2w = torch.cat([A, torch.randn(3, 1, generator=g)], 1).contiguous()
    for _ in range(50):
        dots = normals_dots(quats, scales, means, c2w)
        bad = np.abs(dots) < 0.05
        if not bad.any():
            break
        means[torch.from_numpy(bad)] = torch.randn(int(bad.sum()), 3, generator=g) * 10
    vis = sorted_subset(N, rows, rows + 1)
    G = torch.randn(rows, RS, generator=g)
    return {"quats": quats, "scales": scales, "means": means, "c2w": c2w, "vis": vis, "G": G, "N": N}


def normals_dots(quats, scales, means, c2w):
    """dot(n0, normalize(cam - mean)) per Gaussian in float64 (NaN where the camera sits at the mean)."""
    q, k, _, rows, _, n0, _, _ = no._forward(quats.numpy(), scales.numpy(), means.numpy(), c2w.numpy())
    d = c2w.numpy().astype(np.float64)[:, 3][None] - means.numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (n0 * (d / np.linalg.norm(d, axis=-1, keepdims=True))).sum(-1)


def scale_gaps(scales):
    """Smallest relative distance between two scales of a Gaussian, exact ties left out (inf where all three are tied)."""
    s = scales.double()
    out = torch.full((s.shape[0],), float("inf"), dtype=torch.float64)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        gap = (s[:, a] - s[:, b]).abs() / torch.maximum(s[:, a].abs(), s[:, b].abs())
        out = torch.minimum(out, torch.where(gap == 0, torch.full_like(gap, float("inf")), gap))
    return out


def normals_special():
    """Rows written by hand (CPU float32): scale ties, the camera at a mean, a zero quaternion (column (1, 0, 0): finite), a
    quaternion whose selected column vanishes (the 1e-12 clamp: a zero normal), an unnormalised quaternion.  Returns the scene
    and the expected argmin per row."""
    c2w = torch.tensor([[0.0, -1.0, 0.0, 1.5], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, 0.25]])
    q = torch.tensor([[0.9, 0.1, -0.3, 0.2]] * 4 + [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [3.0, -1.0, 2.0, 0.5], [0.5, 0.5, 0.5, 0.5]])
    s = torch.tensor([[0.5, 0.5, 2.0], [3.0, 0.7, 0.7], [1.1, 1.1, 1.1], [2.0, 1.0, 0.5], [0.1, 1.0, 1.0], [0.1, 1.0, 1.0], [1.0, 0.2, 3.0],
                      [0.3, 0.3, 0.3]])
    m = torch.tensor([[4.0, 1.0, -3.0], [-2.0, 5.0, 1.0], [0.5, 0.5, 8.0], [1.5, -2.0, 0.25], [3.0, 3.0, 3.0], [-1.0, 2.0, 4.0],
                      [6.0, -1.0, 2.0], [-3.0, -3.0, 1.0]])       # row 3: the camera position itself
    k = [0, 1, 0, 2, 0, 0, 1, 0]
    return {"quats": q, "scales": s, "means": m, "c2w": c2w, "N": 8}, k


def normals_plain(quats, scales, means, c2w):
    """The camera-space normals written out row by row in float64 (first of equal minima; `dot < 0` is false for NaN; the
    1e-12 clamp of F.normalize): the plain restatement for the special rows."""
    out = np.zeros((quats.shape[0], 3))
    C = c2w.double().numpy()
    for i in range(quats.shape[0]):
        w, x, y, z = quats[i].double().tolist()
        s = scales[i].double().tolist()
        k = 0
        for j in (1, 2):
            if s[j] < s[k]:
                k = j
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                       [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        col = Rm[:, k]
        n0 = col / max(np.linalg.norm(col), 1e-12)
        d = C[:, 3] - means[i].double().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            dot = float(n0 @ (d / np.linalg.norm(d)))
        out[i] = (-n0 if dot < 0 else n0) @ C[:, :3]
    return out
