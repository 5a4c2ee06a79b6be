"""The colour kernels of the VISIBLE rows called directly (csrc/viscolor.hip, wild.hip visible-row form, normals.hip row forms)
at row, workgroup, count and node-table edges, against the float64 references of tests/row_refs.py.

All cases are tiny and chosen for launch geometry: 16-lane rows and 64-row workgroups of the SH kernels, 32-row MFMA tiles and the
8192-row grid edge of the appearance MLP, 256-row blocks of the normals.  The poison rule holds for every call: outputs are
pre-filled with a recognisable NaN pattern; rows at or past the device count, the geometry floats 0..7 of a record, channels the
call does not own and Gaussians outside vis_ids must come back bit-identical.  Every buffer is allocated with valid guard rows
behind `cap` (in-range Gaussian indices, poisoned outputs), which must come back untouched as well.

Conditioning (tests/test_row_refs_host.py asserts it for every case, without a GPU): no clamp pre-activation within 1e-5 of an
edge except the deliberate float32 edge rows, no ReLU kink on a row with a cotangent, no normal flip with |dot| < 1e-3 -- so masks
and zero patterns are compared for identity and no row is left out.

Tolerances: values and coefficient gradients atol 2e-6 / rtol 1e-5, direction gradients atol 5e-6 / rtol 1e-4
(tests/test_gpu_parity.py::test_sh_fwd_bwd); normals 2e-6 and 2e-5 relative (tests/test_gpu_normals.py); appearance colours 1e-5
and feature gradients 1e-4 of the maximum (tests/test_gpu_wild.py); MLP weight gradients and dir_part: the per-element float32
bounds C_WILD and C_DIR of tests/row_refs.py (measured on the CPU, times 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import row_refs as R

pytestmark = pytest.mark.gpu

RS, COL = R.RS, R.COL
MASK_POISON = 0xA5
BUILT_BY = set()      # how the node tables of this session were built (ShDevice)
bits = R.bits


def _call(name, *a):
    from mtgs_amd import wrapper
    wrapper.call(name, *a)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _zero_bits(t):
    return not bool(bits(t).any())


def _close(got, want, atol, rtol):
    got, want = got.detach().double().cpu(), want.double()
    bad = (got - want).abs() > atol + rtol * want.abs()
    assert not bool(bad.any()), float(((got - want).abs() - rtol * want.abs()).max())


# ---- SH rows --------------------------------------------------------------------------------------------------------------------
class ShDevice:
    """A scene of tests/row_refs.py on the device: one storage tensor per coefficient kind (row strides larger than the row when
    `strided`), NaN in every float the kernels have no business reading: the padding of a row and the coefficients past
    min(k_rest, (degree + 1)^2 - 1) (all of `rest` in a sigmoid node)."""

    def __init__(self, sc, strided=False, nodes=None, dead=None):
        N, self.sc = sc["N"], sc
        dcs, adds, rs = (7, 5, 50) if strided else (3, 3, 45)
        self.dcS, self.restS = R.poisoned((N, dcs), "cuda"), R.poisoned((N, rs), "cuda")
        self.dcS[:, :3] = sc["dc"].cuda()
        self.addS = None
        if sc["add"] is not None:
            self.addS = R.poisoned((N, adds), "cuda")
            self.addS[:, :3] = sc["add"].cuda()
        live = torch.minimum(sc["k_rest"], torch.full_like(sc["k_rest"], (sc["degree"] + 1) ** 2 - 1))
        live = torch.where(sc["use_sh"] == 0, torch.zeros_like(live), live)
        keep = (torch.arange(45)[None] < 3 * live[:, None]).cuda()
        self.restS[:, :45] = torch.where(keep, sc["rest"].reshape(N, 45).cuda(), self.restS[:, :45])
        if dead is not None:      # Gaussians of which NOTHING may be read (flagged-off rows)
            for t in (self.dcS, self.addS, self.restS):
                if t is not None:
                    t[dead.cuda()] = R.poisoned((1,), "cuda")
        self.nodes = nodes or sc["nodes"]
        self.means, self.cam = sc["means"].cuda(), sc["cam"].cuda()
        self.built_by = self._public_table(strided, dead)
        if self.built_by is None:
            self.built_by = "raw"
            self.table = R.node_table(self.nodes, self.dcS, self.addS, self.restS, torch.device("cuda"))
        BUILT_BY.add(self.built_by)

    def _public_table(self, strided, dead):
        """The node table through the public constructors wherever they can express the case (they fill first_block, the strides
        and dc_add_stride as production does): collect_gaussians(..., deferred_colors=True) for one or two non-empty nodes of one
        activation 0 / 1 whose coefficient count covers the degree; sh_coefficient_source for one clamp_min node without dc_add
        (any K).  Everything else -- larger row strides, k_rest below the degree, many or empty nodes -- needs a raw table."""
        from mtgs_amd import nodes as nd
        sc, N = self.sc, self.sc["N"]
        kinds = {u for _, _, _, u in self.nodes}
        if strided or dead is not None or len(self.nodes) > 2 or len(kinds) != 1 or any(n == 0 for _, n, _, _ in self.nodes):
            return None
        use_sh, NB = kinds.pop(), (sc["degree"] + 1) ** 2
        if use_sh == 4 and len(self.nodes) == 1 and self.addS is None:
            K = self.nodes[0][2] + 1
            self._coeffs = torch.cat([self.dcS[:, None, :3], self.restS[:, :45].reshape(N, 15, 3)], 1)[:, :K].contiguous()
            cs = nd.sh_coefficient_source(self._coeffs, sc["degree"], self.cam)
            assert torch.equal(cs.cam, self.cam)
            self._cs, self.table = cs, cs.table
            return "sh_coefficient_source"
        if use_sh in (0, 1) and (use_sh == 0 or all(NB <= k + 1 for _, _, k, _ in self.nodes)):
            g = torch.Generator().manual_seed(5)
            raw = []
            for s0, n, k, _ in self.nodes:
                raw.append({"means": self.means[s0:s0 + n].contiguous(), "scales": torch.randn(n, 3, generator=g).cuda(),
                            "quats": torch.randn(n, 4, generator=g).cuda(), "opacities": torch.randn(n, 1, generator=g).cuda(),
                            "features_dc": self.dcS[s0:s0 + n, :3].contiguous(),
                            "features_rest": self.restS[s0:s0 + n, :3 * k].reshape(n, k, 3).contiguous()})
                if self.addS is not None:
                    raw[-1]["features_adapters"] = self.addS[s0:s0 + n, :3].contiguous()
            c2w = torch.eye(4, device="cuda")[None, :3].clone()
            c2w[0, :, 3] = self.cam
            out = nd.collect_gaussians(raw, c2w, sc["degree"], model_sh_degree=3 if use_sh else 0, deferred_colors=True)
            cs = out["color_source"]
            assert cs.n_nodes == len(self.nodes) and torch.equal(bits(out["means"]), bits(self.means)) and torch.equal(cs.cam, self.cam)
            self._cs, self._raw, self.table = cs, raw, cs.table
            return "collect_gaussians"
        return None


    def fwd(self, ids, totals, cap, recs, vmask, coef=None, flags=None, dirs=None, means=None):
        means = self.means if means is None else means
        if dirs is None:
            _call("mtgs_vis_color_fwd", len(self.nodes), _ptr(self.table), self.sc["degree"], _ptr(self.cam), _ptr(means), _ptr(ids), _ptr(totals),
                  cap, _ptr(recs), _ptr(vmask), _ptr(coef), 0 if coef is None else coef.stride(0), _ptr(flags), _st())
        else:
            _call("mtgs_vis_color_fwd_dirs", len(self.nodes), _ptr(self.table), self.sc["degree"], None, None, _ptr(ids), _ptr(totals), cap,
                  _ptr(recs), _ptr(vmask), _ptr(coef), 0 if coef is None else coef.stride(0), _ptr(flags), _ptr(dirs), _st())

    def bwd(self, ids, totals, cap, G, recs, vmask, feat, dir_rows, dir_part, dense=None, dirs=None, means=None):
        means = self.means if means is None else means
        if dirs is None:
            _call("mtgs_vis_color_bwd", len(self.nodes), _ptr(self.table), self.sc["degree"], _ptr(self.cam), _ptr(means), _ptr(ids), _ptr(totals),
                  cap, _ptr(G), G.stride(0), COL, _ptr(recs), _ptr(vmask), _ptr(feat), _ptr(dir_rows), _ptr(dir_part), _ptr(dense), _st())
        else:
            _call("mtgs_vis_color_bwd_dirs", len(self.nodes), _ptr(self.table), self.sc["degree"], None, None, _ptr(ids), _ptr(totals), cap,
                  _ptr(G), G.stride(0), COL, _ptr(recs), _ptr(vmask), _ptr(feat), _ptr(dir_rows), _ptr(dir_part), _ptr(dense), _ptr(dirs), _st())


def _buffers(sc, cap):
    alloc = (cap // 64 + 2) * 64
    ids = R.padded_ids(sc["vis"], sc["N"], alloc).cuda()
    recs = R.poisoned((alloc, R.REC), "cuda")
    vmask = torch.full((alloc,), MASK_POISON, dtype=torch.uint8, device="cuda")
    return alloc, ids, recs, vmask


def _run_sh(dev, cap_extra=0, tot_extra=0, **kw):
    """Forward and both backward forms of a scene with every poison check; returns the outputs for further comparisons."""
    sc = dev.sc
    n = sc["vis"].numel()
    cap = n + cap_extra
    alloc, ids, recs, vmask = _buffers(sc, cap)
    totals = R.totals_word(n + tot_extra, "cuda")
    dev.fwd(ids, totals, cap, recs, vmask, **kw)
    assert bool(R.is_poison(recs[n:]).all()) and bool((vmask[n:] == MASK_POISON).all()), "rows at or past the count were written"
    assert bool(R.is_poison(recs[:n, :8]).all()) and bool(R.is_poison(recs[:n, 11:]).all()), "floats outside channels 0..2 were written"
    G = R.grad_rows(sc["cot"], alloc, RS, COL).cuda()
    blocks = alloc // 64
    feat, drows, dpart = R.poisoned((alloc, 48), "cuda"), R.poisoned((alloc, 3), "cuda"), torch.zeros(blocks, 3, device="cuda")
    dev.bwd(ids, totals, cap, G, recs, vmask, feat, drows, dpart, **kw)
    assert bool(R.is_poison(feat[n:]).all()) and bool(R.is_poison(drows[n:]).all())
    used = -(-n // 64)
    assert _zero_bits(dpart[used:]), "dir_part of a workgroup past the count was written"
    # dense_rows: the rows with a cotangent, bit for bit, into the zeroed [N, 16, 3] gradient; nothing else, and no feat_rows
    dense, feat2 = torch.zeros(sc["N"], 48, device="cuda"), R.poisoned((alloc, 48), "cuda")
    drows2, dpart2 = R.poisoned((alloc, 3), "cuda"), torch.zeros(blocks, 3, device="cuda")
    dev.bwd(ids, totals, cap, G, recs, vmask, feat2, drows2, dpart2, dense=dense, **kw)
    assert bool(R.is_poison(feat2).all())
    assert torch.equal(bits(drows2), bits(drows)) and torch.equal(bits(dpart2), bits(dpart))
    v = sc["vis"].long().cuda()
    has = (feat[:n] != 0).any(1)
    assert torch.equal(bits(dense[v][has]), bits(feat[:n][has]))
    rest = torch.ones(sc["N"], dtype=torch.bool, device="cuda")
    rest[v[has]] = False
    assert _zero_bits(dense[rest])
    return {"n": n, "recs": recs, "vmask": vmask, "feat": feat, "drows": drows, "dpart": dpart, "ids": ids, "G": G, "totals": totals,
            "cap": cap, "alloc": alloc}


def _check_sh(out, sc, ref, flags=None):
    """The outputs of _run_sh against the float64 reference of the scene (rows flagged off: the documented constants)."""
    n = out["n"]
    on = torch.ones(n, dtype=torch.bool) if flags is None else flags[:n].bool().cpu()
    col = out["recs"][:n, 8:11].cpu()
    _close(col[on], ref["colour"][on], 2e-6, 1e-5)
    assert torch.equal(out["vmask"][:n].cpu()[on], ref["mask"][on]), "clamp pass-through bits"
    if not bool(on.all()):
        assert bool((col[~on] == 0.5).all()) and bool((out["vmask"][:n].cpu()[~on] == 7).all())
        return
    feat = out["feat"][:n].cpu().reshape(n, 16, 3)
    _close(feat, ref["feat"], 2e-6, 1e-5)
    assert not bool(feat[ref["feat"] == 0].any()), "a column past the degree / k_rest, a masked channel or a zero-cotangent row is not exactly zero"
    _close(out["drows"][:n], ref["ddir"], 5e-6, 1e-4)
    zero = (sc["cot"] == 0).all(-1)
    assert not bool(out["drows"][:n].cpu()[zero].any()), "the direction gradient of a zero-cotangent row is not exactly zero"
    part = out["dpart"].double().cpu()
    for b in range(-(-n // 64)):
        want, bound = ref["ddir"][64 * b:64 * b + 64].sum(0), R.C_DIR * R.U32 * ref["dterms"][64 * b:64 * b + 64].sum(0)
        assert bool(((part[b] - want).abs() <= bound).all()), (b, ((part[b] - want).abs() / bound.clamp_min(1e-300)).max())
    total, bound = ref["ddir"].sum(0), R.C_DIR * R.U32 * ref["dterms"].sum(0)
    assert bool(((part.sum(0) - total).abs() <= bound).all())


@pytest.mark.parametrize("case", R.SH_CASES, ids=[c[0] for c in R.SH_CASES])
def test_sh_rows_sizes_and_options(hip_lib, case):
    name, n_rows, cap_extra, tot_extra, degree, k_rest, use_sh, add, strided, n_nodes = case
    sc = R.sh_scene(name, n_rows, degree, k_rest, use_sh, add, n_nodes)
    out = _run_sh(ShDevice(sc, strided), cap_extra, tot_extra)
    _check_sh(out, sc, R.sh_scene_ref(sc))


@pytest.mark.parametrize("use_sh", [1, 4])
def test_sh_rows_clamp_edges(hip_lib, use_sh):
    """Pre-activations exactly 0 and 1 and their float32 neighbours: the mask bits are the inclusive float32 decision."""
    sc = R.sh_edge_scene(use_sh)
    ref = R.sh_scene_ref(sc)
    out = _run_sh(ShDevice(sc), 0, 0)
    _check_sh(out, sc, ref)
    assert torch.equal(bits(out["recs"][:6, 8]), bits(ref["pre32"][:6, 0].clamp(0, 1) if use_sh == 1 else ref["pre32"][:6, 0].clamp_min(0)))


def test_sh_rows_node_tables_128_and_129(hip_lib):
    """The binary search over `start`: 129 nodes (global memory) and 128 (LDS) of mostly 1 to 3 Gaussians with empty nodes in front,
    in the middle and behind; every node has its own (k_rest, use_sh), so a Gaussian resolved to a neighbour gets another colour."""
    sc = R.sh_table_scene()
    ref = R.sh_scene_ref(sc)
    a = _run_sh(ShDevice(sc, True), 3, 0)
    _check_sh(a, sc, ref)
    b = _run_sh(ShDevice(sc, True, nodes=sc["nodes128"]), 3, 0)
    for k in ("recs", "feat", "drows", "dpart"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(a["vmask"], b["vmask"])


@pytest.mark.parametrize("use_sh", R.OPT_USE_SH)
def test_sh_rows_coef_rows_flags_dirs_and_zero_cotangents(hip_lib, use_sh):
    sc = R.sh_opts_scene(use_sh)
    ref = R.sh_scene_ref(sc)
    dev = ShDevice(sc, True)
    base = _run_sh(dev, 3, 0)
    _check_sh(base, sc, ref)
    n, cap, alloc, ids, totals = base["n"], base["cap"], base["alloc"], base["ids"], base["totals"]
    v = sc["vis"].long()
    # coef_rows: the compact rows [dc 3 | dc_add 3 | rest 45 | pad] instead of the parameters in place
    coef = R.poisoned((alloc, 52), "cuda")
    coef[:n, 0:3], coef[:n, 3:6], coef[:n, 6:51] = sc["dc"][v].cuda(), sc["add"][v].cuda(), dev.restS[v.cuda(), :45]
    recs, vmask = R.poisoned((alloc, R.REC), "cuda"), torch.full((alloc,), MASK_POISON, dtype=torch.uint8, device="cuda")
    dev.fwd(ids, totals, cap, recs, vmask, coef=coef)
    assert torch.equal(bits(recs), bits(base["recs"])) and torch.equal(vmask, base["vmask"])
    # caller-supplied directions == means - cam
    dirs = dev.means - dev.cam
    d = _run_sh(dev, 3, 0, dirs=dirs)
    for k in ("recs", "feat", "drows", "dpart"):
        assert torch.equal(bits(d[k]), bits(base[k])), k
    # row_flags: a third of the rows off; nothing of them is read (coefficients and means NaN), the record holds 0.5, the mask 7
    flags = torch.ones(alloc, dtype=torch.uint8)
    flags[:n][torch.arange(n) % 3 == 1] = 0
    off = v[flags[:n] == 0]
    dead = ShDevice(sc, True, dead=off)
    means = dev.means.clone()
    means[off.cuda()] = R.poisoned((1,), "cuda")
    recs, vmask = R.poisoned((alloc, R.REC), "cuda"), torch.full((alloc,), MASK_POISON, dtype=torch.uint8, device="cuda")
    dead.fwd(ids, totals, cap, recs, vmask, flags=flags.cuda(), means=means)
    _check_sh({"n": n, "recs": recs, "vmask": vmask}, sc, ref, flags=flags)
    on = (flags[:n] == 1).cuda()
    assert torch.equal(bits(recs[:n][on]), bits(base["recs"][:n][on])) and bool(R.is_poison(recs[n:]).all())
    assert bool(R.is_poison(recs[:n, :8]).all()) and bool(R.is_poison(recs[:n, 11:]).all()) and bool((vmask[n:] == MASK_POISON).all())
    # zero-cotangent rows (and those below the flush threshold... which do fetch): the direction of an exactly-zero row is not read
    zero = (sc["cot"] == 0).all(-1)
    means = dev.means.clone()
    means[v[zero].cuda()] = R.poisoned((1,), "cuda")
    feat, drows, dpart = R.poisoned((alloc, 48), "cuda"), R.poisoned((alloc, 3), "cuda"), torch.zeros(alloc // 64, 3, device="cuda")
    dev.bwd(ids, totals, cap, base["G"], base["recs"], base["vmask"], feat, drows, dpart, means=means)
    for k, t in (("feat", feat), ("drows", drows), ("dpart", dpart)):
        assert torch.equal(bits(t), bits(base[k])), k
    assert not bool(feat[:n][zero.cuda()].any()) and not bool(drows[:n][zero.cuda()].any())


@pytest.mark.parametrize("use_sh,K", R.TWIN_CASES)
def test_sh_rows_equal_the_dense_twin(hip_lib, use_sh, K):
    """Tables from the public constructors (sh_direction_source: two K = 16 nodes with the caller's directions; sh_coefficient_source:
    one [N, K, 3] tensor, K < 16 gives k_rest < 15 and a short row stride).  K = 16: the same bits as the dense kernel with the
    activation fused (mtgs_sh_fwd_act), colours and pass-through bits; K < 16: the float64 reference."""
    from mtgs_amd.nodes import sh_coefficient_source, sh_direction_source
    sc = R.sh_twin_scene(use_sh, K)
    N, n, degree = sc["N"], 70, sc["degree"]
    coeffs = torch.cat([sc["dc"][:, None], sc["rest"]], 1)[:, :K].contiguous().cuda()
    dirs = (sc["means"] - sc["cam"]).cuda()
    if use_sh == 1:
        cut = sc["nodes"][0][1]
        cs = sh_direction_source([coeffs[:cut], coeffs[cut:]], degree, [dirs[:cut], dirs[cut:]], 1)
    else:
        cs = sh_coefficient_source(coeffs, degree, sc["cam"].cuda())
    alloc, ids, recs, vmask = _buffers(sc, n)
    totals, means = R.totals_word(n, "cuda"), sc["means"].cuda()
    _call("mtgs_vis_color_fwd_dirs", cs.n_nodes, _ptr(cs.table), cs.degree, _ptr(cs.cam), _ptr(means), _ptr(ids), _ptr(totals), n,
          _ptr(recs), _ptr(vmask), None, 0, None, _ptr(cs.dirs), _st())
    ref = R.sh_scene_ref(sc)
    _close(recs[:n, 8:11], ref["colour"], 2e-6, 1e-5)
    assert torch.equal(vmask[:n].cpu(), ref["mask"]) and bool(R.is_poison(recs[n:]).all())
    v = sc["vis"].long().cuda()
    # backward: the coefficient-gradient rows against the dense backward with the same pass-through bits (mtgs_sh_bwd_rows_act into
    # a zeroed [N, K, 3]).  It evaluates the basis in gsplat's form, not lane-wise, so this is a float32 twin within the value
    # tolerance, not bit for bit; it has no flush, so the rows below the flush threshold are compared with zero instead.
    G = R.grad_rows(sc["cot"], alloc, RS, COL).cuda()
    feat = R.poisoned((alloc, 48), "cuda")
    _call("mtgs_vis_color_bwd_dirs", cs.n_nodes, _ptr(cs.table), cs.degree, _ptr(cs.cam), _ptr(means), _ptr(ids), _ptr(totals), n, _ptr(G), RS,
          COL, _ptr(recs), _ptr(vmask), _ptr(feat), None, None, None, _ptr(cs.dirs), _st())
    assert bool(R.is_poison(feat[n:]).all())
    _close(feat[:n].reshape(n, 16, 3), ref["feat"], 2e-6, 1e-5)
    V, passed_all = torch.zeros(N, 3, device="cuda"), torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    V[v], passed_all[v] = G[:n, COL:COL + 3], vmask[:n]
    twin = torch.zeros(N, K, 3, device="cuda")
    _call("mtgs_sh_bwd_rows_act", N, K, degree, _ptr(dirs), None, _ptr(V), _ptr(twin), _ptr(passed_all), _st())
    flushed = ((sc["cot"].abs() < R.FLUSH) & (sc["cot"] != 0)).any(-1).cuda()
    assert not bool(feat[:n][flushed].any())
    _close(feat[:n].reshape(n, 16, 3)[~flushed][:, :K], twin[v][~flushed].cpu(), 2e-6, 1e-5)
    assert not bool(feat[:n].reshape(n, 16, 3)[:, K:].any())
    if K == 16:
        from mtgs_amd.wrapper import _SphericalHarmonics
        col, passed = torch.empty(N, 3, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
        _call("mtgs_sh_fwd_act", N, 16, degree, _ptr(dirs), _ptr(coeffs), None, _ptr(col), 1, 0.5, 0.0, 1.0 if use_sh == 1 else float("inf"),
              _ptr(passed), _st())
        assert torch.equal(bits(recs[:n, 8:11]), bits(col[v])) and torch.equal(vmask[:n], passed[v])
        # spherical_harmonics() and the caller's own activation as separate kernels
        sh = _SphericalHarmonics.apply(degree, dirs, coeffs, None) + 0.5
        sep = torch.clamp(sh, 0.0, 1.0) if use_sh == 1 else torch.clamp_min(sh, 0.0)
        assert torch.equal(bits(recs[:n, 8:11]), bits(sep[v]))


def test_sh_tables_came_from_every_builder(hip_lib):
    """The SH cases above built their node tables through collect_gaussians(deferred_colors=True), sh_coefficient_source and raw
    descriptors (sh_direction_source: the twin test)."""
    for case in R.SH_CASES:
        name, n_rows, _, _, degree, k_rest, use_sh, add, strided, n_nodes = case
        ShDevice(R.sh_scene(name, n_rows, degree, k_rest, use_sh, add, n_nodes), strided)
    assert BUILT_BY >= {"collect_gaussians", "sh_coefficient_source", "raw"}, BUILT_BY


@pytest.mark.parametrize("N,width,stride", R.EXPAND_CASES)
@pytest.mark.parametrize("rows", ["none", "all", "mixed"])
def test_rows_expand(hip_lib, N, width, stride, rows):
    g = torch.Generator().manual_seed(N * 7 + width)
    n_rows = max(N // 2, 1)
    src = torch.randn(n_rows, stride, generator=g).cuda()
    row_of = torch.randint(0, n_rows, (N,), generator=g, dtype=torch.int32)
    if rows == "none":
        row_of[:] = -1
    elif rows == "mixed":
        row_of[torch.arange(N) % 3 == 0] = -1
    out, row_dev = R.poisoned((N + 3, width), "cuda"), row_of.cuda()
    _call("mtgs_rows_expand", N, width, _ptr(row_dev), _ptr(src), stride, _ptr(out), _st())
    want = torch.where((row_of >= 0)[:, None].cuda(), src[row_of.clamp_min(0).long().cuda(), :width], torch.zeros(N, width, device="cuda"))
    assert torch.equal(bits(out[:N]), bits(want)) and bool(R.is_poison(out[N:]).all())


# ---- appearance MLP -------------------------------------------------------------------------------------------------------------
_wild_dev = {}


def _wild(with_emb):
    """The parameter set on the device, the dense colours and feature gradients of ALL Gaussians (one launch each) and the float64
    colours: computed once, shared, never changed."""
    if with_emb not in _wild_dev:
        from mtgs_amd import appearance as A
        ts, cot, _ = R.wild_case(with_emb)
        dts = [None if t is None else t.cuda() for t in ts]
        prep = A._prepared(dts[0], dts[1], dts[2], dts[3:])
        out = torch.empty(R.WILD_N, 3, device="cuda")
        A._forward(prep, R.WILD_N, None, None, None, out, 3, _st())
        g = cot.cuda()
        shapes = (dts[0].shape, dts[1].shape, None if dts[2] is None else dts[2].shape)
        grads = A._backward(prep, shapes, (True,) * 9, R.WILD_N, None, None, g.data_ptr(), 3, _st())
        with torch.no_grad():
            ref = R.wild_reference(ts)
        _wild_dev[with_emb] = {"ts": ts, "dts": dts, "prep": prep, "cot": cot, "colour": out, "grads": grads, "ref": ref, "g": g}
    return _wild_dev[with_emb]


def _wild_ids(alloc):
    """vis_ids of alloc rows: the odd Gaussians, then (guard rows) even ones -- all in range, none twice."""
    odd = R.wild_vis_ids(min(alloc, 8226))
    return torch.cat([odd, torch.arange(alloc - odd.numel(), dtype=torch.int32) * 2]).cuda()


@pytest.mark.parametrize("with_emb", [True, False])
def test_wild_dense_all_against_float64(hip_lib, with_emb):
    w = _wild(with_emb)
    assert float((w["colour"].double().cpu() - w["ref"]).abs().max()) <= 1e-5
    g64, _ = R.wild_backward_ref(w["ts"], w["cot"])
    for i, name in enumerate(R.WILD_NAMES[:2]):
        got, want = w["grads"][i].double().cpu(), g64[name]
        assert float((got - want).abs().max()) <= 1e-4 * float(want.abs().max()), name
    assert not bool(w["grads"][1].reshape(R.WILD_N, 45)[:, 24:].any())


@pytest.mark.parametrize("rows", R.WILD_ROWS)
def test_wild_rows_are_independent_of_form_position_and_count(hip_lib, rows):
    """A Gaussian's colour and feature gradients have the same bits in the dense form over all Gaussians, over a prefix of `rows`
    Gaussians, and in the visible-row form at cap == / > / < totals, with other rows flagged off, through out_stride 3 and through
    WildColorSource into the records; totals == 0 writes nothing."""
    from mtgs_amd import appearance as A
    w = _wild(True)
    prep, dts = w["prep"], w["dts"]
    # dense over the first `rows` Gaussians
    out = R.poisoned((rows + 40, 3), "cuda")
    sub = A._prepared(dts[0][:rows], dts[1][:rows], dts[2], dts[3:])
    A._forward(sub, rows, None, None, None, out, 3, _st())
    assert torch.equal(bits(out[:rows]), bits(w["colour"][:rows])) and bool(R.is_poison(out[rows:]).all())
    alloc = rows + 104
    ids = _wild_ids(alloc)
    src = A.WildColorSource(dts[0], dts[1], dts[2], dts[3:])
    for cap, tot in ((rows, rows), (rows + 40, rows), (rows, rows + 9), (rows + 40, 0)):
        n = min(cap, tot)
        totals = R.totals_word(tot, "cuda")
        recs = R.poisoned((alloc, R.REC), "cuda")
        src.colour_rows(ids, totals, cap, recs, None, _st())
        want = w["colour"][ids[:n].long()]
        assert torch.equal(bits(recs[:n, 8:11]), bits(want)), (cap, tot)
        assert bool(R.is_poison(recs[n:]).all()) and bool(R.is_poison(recs[:n, :8]).all()) and bool(R.is_poison(recs[:n, 11:]).all()), (cap, tot)
        out3 = R.poisoned((alloc, 3), "cuda")
        A._forward(prep, cap, ids, totals, None, out3, 3, _st())
        assert torch.equal(bits(out3[:n]), bits(want)) and bool(R.is_poison(out3[n:]).all())
        # rows flagged off: zeros; the others keep their bits
        flags = (torch.arange(alloc) % 3 != 1).to(torch.uint8).cuda()
        recs = R.poisoned((alloc, R.REC), "cuda")
        src.colour_rows(ids, totals, cap, recs, flags, _st())
        on = flags[:n].bool()
        assert torch.equal(bits(recs[:n, 8:11][on]), bits(want[on])) and _zero_bits(recs[:n, 8:11][~on])
        assert bool(R.is_poison(recs[n:]).all()) and bool(R.is_poison(recs[:n, :8]).all()) and bool(R.is_poison(recs[:n, 11:]).all())
        # backward through the source: grad_stride = RS, colour columns at 8
        G = R.grad_rows(w["cot"][ids[:n].long().cpu()], alloc, RS, COL).cuda()
        grads = src.backward_rows((True,) * 9, ids, totals, cap, G, RS, _st())
        seen = torch.zeros(R.WILD_N, dtype=torch.bool, device="cuda")
        seen[ids[:n].long()] = True
        for got, full in ((grads[0], w["grads"][0]), (grads[1].reshape(R.WILD_N, 45), w["grads"][1].reshape(R.WILD_N, 45))):
            assert torch.equal(bits(got[seen]), bits(full[seen])), (cap, tot)
            assert _zero_bits(got[~seen]), "a Gaussian outside the visible rows got a feature gradient"
        assert not bool(grads[1].reshape(R.WILD_N, 45)[:, 24:].any())
        if cap > 0:      # the kernel itself, into poisoned gradients: only the Gaussians of the first n rows are written
            d_dc, d_rest, nbytes = R.poisoned((R.WILD_N, 3), "cuda"), R.poisoned((R.WILD_N, 45), "cuda"), C.c_size_t(0)
            _call("mtgs_wild_workspace_bytes", cap, C.byref(nbytes))
            part = torch.empty(nbytes.value // 4, device="cuda")
            _call("mtgs_wild_bwd", cap, _ptr(ids), _ptr(totals), G.data_ptr() + 4 * COL, RS, _ptr(prep[0]), prep[0].stride(0), _ptr(prep[1]),
                  prep[1].stride(0), *(_ptr(t) for t in prep[2:]), *A._widths(), _ptr(d_dc), _ptr(d_rest), 45, _ptr(part), nbytes.value, _st())
            assert torch.equal(bits(d_dc[seen]), bits(w["grads"][0][seen])) and bool(R.is_poison(d_dc[~seen]).all()), (cap, tot)
            assert torch.equal(bits(d_rest[seen]), bits(w["grads"][1].reshape(R.WILD_N, 45)[seen])) and bool(R.is_poison(d_rest[~seen]).all())
        if n == 0:
            assert all(not bool(g.any()) for g in grads[2:])


@pytest.mark.parametrize("with_emb", [True, False])
@pytest.mark.parametrize("rows", R.WILD_GRAD_ROWS)
def test_wild_weight_gradients(hip_lib, rows, with_emb):
    """Per element against float64 within C_WILD 2^-24 sum |term|; bitwise equal between two runs; the dense form over the same
    rows within the same bound of the visible form (another order of partials)."""
    from mtgs_amd import appearance as A
    w = _wild(with_emb)
    dts = w["dts"]
    alloc = rows + 72
    ids = _wild_ids(alloc)
    v = ids[:rows].long()
    totals = R.totals_word(rows, "cuda")
    G = R.grad_rows(w["cot"][v.cpu()], alloc, RS, COL).cuda()
    src = A.WildColorSource(dts[0], dts[1], dts[2], dts[3:])
    runs = [src.backward_rows((True,) * 9, ids, totals, rows + 40, G, RS, _st()) for _ in range(2)]
    sub_ts = [None if t is None else (t[v.cpu()] if i < 2 else t) for i, t in enumerate(w["ts"])]
    g64, terms = R.wild_backward_ref(sub_ts, w["cot"][v.cpu()])
    sub = A._prepared(dts[0][v], dts[1][v], dts[2], dts[3:])
    shapes = (sub[0].shape, (rows, 15, 3), None if dts[2] is None else dts[2].shape)
    gc = G[:rows, COL:COL + 3].contiguous()
    dense = A._backward(sub, shapes, (True,) * 9, rows, None, None, gc.data_ptr(), 3, _st())
    for i, name in enumerate(R.WILD_NAMES):
        if i < 2:
            continue
        if name == "embedding" and not with_emb:
            assert runs[0][i] is None
            continue
        a, b, d = runs[0][i], runs[1][i], dense[i]
        assert torch.equal(bits(a), bits(b)), name
        bound = R.C_WILD * R.U32 * terms[name]
        err = (a.double().cpu() - g64[name]).abs()
        assert bool((err <= bound).all()), (name, float((err / (R.U32 * terms[name]).clamp_min(1e-300)).max()))
        assert bool(((a.double() - d.double()).abs().cpu() <= bound).all()), name
    if not with_emb:
        assert _zero_bits(runs[0][3][:, 27:])


# ---- normals --------------------------------------------------------------------------------------------------------------------
NCOL = 11      # the normal cotangent in the gradient rows: behind the three colour columns


def _normals_dense(sc, V=None):
    q, s, m, c = (sc[k].cuda() for k in ("quats", "scales", "means", "c2w"))
    N = sc["N"]
    out = R.poisoned((N + 2, 3), "cuda")
    _call("mtgs_normals_fwd", N, _ptr(q), _ptr(s), _ptr(m), _ptr(c), None, _ptr(out), 3, _st())
    assert bool(R.is_poison(out[N:]).all())
    gq = None
    if V is not None:
        gq = R.poisoned((N + 2, 4), "cuda")
        _call("mtgs_normals_bwd", N, _ptr(q), _ptr(s), _ptr(m), _ptr(c), _ptr(V), V.stride(0), _ptr(gq), _st())
        assert bool(R.is_poison(gq[N:]).all())
    return (q, s, m, c), out[:N], None if gq is None else gq[:N]


def _normals_rows(dev, dense, gq, ids, G, cap, tot, n):
    """Every row form at one (cap, totals) against the dense per-Gaussian results, bit for bit, with the poison rule."""
    q, s, m, c = dev
    alloc = ids.numel()
    totals = None if tot is None else R.totals_word(tot, "cuda")
    g = ids[:n].long()
    for channel in (0, 3, 5):
        recs = R.poisoned((alloc, R.REC), "cuda")
        _call("mtgs_normals_fwd_rows", cap, _ptr(ids), _ptr(totals), _ptr(q), _ptr(s), _ptr(m), _ptr(c), _ptr(recs), channel, None, _st())
        own = torch.zeros(R.REC, dtype=torch.bool)
        own[8 + channel:11 + channel] = True
        assert torch.equal(bits(recs[:n][:, own]), bits(dense[g])), (channel, cap, tot)
        assert bool(R.is_poison(recs[n:]).all()) and bool(R.is_poison(recs[:n][:, ~own]).all()), (channel, cap, tot)
    flags = (torch.arange(alloc) % 4 != 2).to(torch.uint8).cuda()
    recs = R.poisoned((alloc, R.REC), "cuda")
    _call("mtgs_normals_fwd_rows", cap, _ptr(ids), _ptr(totals), _ptr(q), _ptr(s), _ptr(m), _ptr(c), _ptr(recs), 3, _ptr(flags), _st())
    on = flags[:n].bool()
    assert torch.equal(bits(recs[:n, 11:14][on]), bits(dense[g][on])) and _zero_bits(recs[:n, 11:14][~on])
    assert bool(R.is_poison(recs[n:]).all()) and bool(R.is_poison(recs[:n, :11]).all()) and bool(R.is_poison(recs[:n, 14:]).all())
    # backward rows: a zero cotangent gives exact zeros, every other row the dense kernel's bits
    qrows = R.poisoned((alloc, 4), "cuda")
    _call("mtgs_normals_bwd_qrows", cap, _ptr(ids), _ptr(totals), _ptr(q), _ptr(s), _ptr(m), _ptr(c), _ptr(G), RS, NCOL, _ptr(qrows), _st())
    zero = (G[:n, NCOL:NCOL + 3] == 0).all(1)
    assert torch.equal(bits(qrows[:n][~zero]), bits(gq[g][~zero])) and _zero_bits(qrows[:n][zero]) and bool(R.is_poison(qrows[n:]).all())
    if tot is None or tot == cap:      # mtgs_normals_bwd_rows takes the count from the host: `w += o` on floats 3..6 of the wire rows
        wire = torch.randn(alloc, 16, generator=torch.Generator().manual_seed(9)).cuda()
        wire[:n:2, 3:7] = 0.0
        before = wire.clone()
        _call("mtgs_normals_bwd_rows", n, _ptr(ids), _ptr(q), _ptr(s), _ptr(m), _ptr(c), _ptr(G), RS, NCOL, _ptr(wire), _st())
        assert torch.equal(bits(wire[:n, 3:7]), bits(before[:n, 3:7] + gq[g])), "wire rows: not `+=` of the dense kernel's gradient"
        assert torch.equal(bits(wire[:n, :3]), bits(before[:n, :3])) and torch.equal(bits(wire[:n, 7:]), bits(before[:n, 7:]))
        assert torch.equal(bits(wire[n:]), bits(before[n:]))


@pytest.mark.parametrize("rows", R.NORMAL_ROWS)
def test_normals_all_entry_points(hip_lib, rows):
    from oracle import normals_oracle as no
    sc = R.normals_scene(rows)
    N = sc["N"]
    alloc = (rows // 256 + 2) * 256
    ids = R.padded_ids(sc["vis"], N, alloc).cuda()
    G = torch.randn(alloc, RS, generator=torch.Generator().manual_seed(rows)).cuda()
    G[torch.arange(alloc) % 4 == 1, NCOL:NCOL + 3] = 0.0
    V = torch.zeros(N, 3, device="cuda")
    V[ids[:rows + 5].long()] = G[:rows + 5, NCOL:NCOL + 3]          # (rows + 5 distinct Gaussians: the largest cap below)
    dev, dense, gq = _normals_dense(sc, V)
    npy = [sc[k].numpy() for k in ("quats", "scales", "means", "c2w")]
    if N:
        assert np.abs(dense.cpu().numpy() - no.normals_fwd(*npy)).max() < 2e-6
        ref_g = no.normals_bwd(*npy, V.cpu().numpy())
        assert np.abs(gq.cpu().numpy() - ref_g).max() < 2e-5 * max(1.0, np.abs(ref_g).max())
    # [rgbs | normals] in one launch
    rgbs = torch.rand(N, 3, generator=torch.Generator().manual_seed(1)).cuda()
    out6 = R.poisoned((N + 1, 6), "cuda")
    _call("mtgs_normals_fwd", N, *(_ptr(t) for t in dev), _ptr(rgbs), _ptr(out6), 6, _st())
    assert torch.equal(bits(out6[:N, 3:]), bits(dense)) and torch.equal(bits(out6[:N, :3]), bits(rgbs)) and bool(R.is_poison(out6[N:]).all())
    for cap, tot in ((rows, None), (rows, rows), (rows + 5, rows), (rows, rows + 7), (rows + 5, None), (rows + 5, 0)):
        n = cap if tot is None else min(cap, tot)
        _normals_rows(dev, dense, gq, ids, G, cap, tot, n)


def test_normals_special_rows(hip_lib):
    """Scale ties give the first minimum, the camera at a mean gives no flip and a finite normal, a zero quaternion and a vanishing
    column stay finite (the 1e-12 clamp), an unnormalised quaternion: all five entry points against the plain restatement."""
    from oracle import normals_oracle as no
    sc, _ = R.normals_special()
    sc["vis"] = torch.arange(8, dtype=torch.int32)
    alloc = 256
    ids = torch.cat([sc["vis"], torch.arange(alloc - 8, dtype=torch.int32) % 8]).cuda()
    G = torch.randn(alloc, RS, generator=torch.Generator().manual_seed(2)).cuda()
    V = G[:8, NCOL:NCOL + 3].contiguous()
    dev, dense, gq = _normals_dense(sc, V)
    want = R.normals_plain(sc["quats"], sc["scales"], sc["means"], sc["c2w"])
    assert bool(torch.isfinite(dense).all()) and bool(torch.isfinite(gq).all())
    assert np.abs(dense.cpu().numpy() - want).max() < 2e-6
    npy = [sc[k].numpy() for k in ("quats", "scales", "means", "c2w")]
    ref_g = no.normals_bwd(*npy, V.cpu().numpy())
    # per row: the vanishing-column row has a gradient of 1e12 (the 1e-12 clamp) and must not set the scale of the others
    assert (np.abs(gq.cpu().numpy() - ref_g) <= 2e-5 * np.maximum(1.0, np.abs(ref_g).max(axis=1, keepdims=True))).all()
    assert np.abs(ref_g[5]).max() > 1e11 and np.abs(ref_g[[0, 1, 2, 3, 6, 7]]).max() < 10
    _normals_rows(dev, dense, gq, ids, G, 8, 8, 8)
    _normals_rows(dev, dense, gq, ids, G, 8, None, 8)
