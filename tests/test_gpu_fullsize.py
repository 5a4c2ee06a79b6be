"""Parity at BASELINE.json's sizes (WB-v1 scenes): the oracle still finishes in seconds on the GPU
box's host cores, so the HIP path is compared with it DIRECTLY at full size, plus the
size-independent properties of the domain (sortedness, offsets, alpha range, absgrad >= |grad|,
determinism of the integer stages, linearity of the backward in the cotangent)."""
import math

import numpy as np
import pytest
import torch

from mtgs_amd.synthetic import make_camera, make_scene
from tests.util import (assert_grad_close, assert_image_close, assert_tile_lists, blend_rows_accounted, listed, moment_xy_terms,
                        projection_vjp_accounted)

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def gs(hip_lib):
    assert torch.cuda.is_available()
    import mtgs_amd
    return mtgs_amd


def test_config1_100k_640x480_forward(gs, oracle):
    """BASELINE configs[0]: 100k Gaussians, 640x480, SH degree 0 (colours given), forward only."""
    N, W, H = 100_000, 640, 480
    sc = make_scene(N, seed=0)
    vm, K = make_camera(W, H)
    a = {k: v.numpy() for k, v in sc.items()}
    r_ref, a_ref, m = oracle.rasterization(a["means"], a["quats"], a["scales"], a["opacities"], a["colors"], vm.numpy(),
                                           K.numpy(), W, H)
    render, alpha, info = gs.rasterization(dev(sc["means"]), dev(sc["quats"]), dev(sc["scales"]), dev(sc["opacities"]),
                                           dev(sc["colors"]), dev(vm), dev(K), W, H, packed=False)
    for key in ("radii", "tiles_per_gauss"):
        assert np.array_equal(info[key].cpu().numpy(), m[key]), key
    assert_tile_lists(info, m, rerun=lambda: gs.rasterization(dev(sc["means"]), dev(sc["quats"]), dev(sc["scales"]), dev(sc["opacities"]),
                                                              dev(sc["colors"]), dev(vm), dev(K), W, H, packed=False)[2])
    for key in ("means2d", "depths", "conics"):
        assert np.array_equal(info[key].cpu().numpy(), m[key]), key
    assert_image_close(render.cpu().numpy(), r_ref, m["critical"], name="render", case="C1 100k 640x480")
    assert_image_close(alpha.cpu().numpy(), a_ref, m["critical"], name="alpha", case="C1 100k 640x480")


@pytest.mark.parametrize("N,sh", [(500_000, True), (2_000_000, False)])
def test_config2_config3_1080p_forward_backward(gs, oracle, N, sh):
    """BASELINE configs[1] (500k, SH degree 3) and configs[2] (2M), 1920x1080, MTGS options
    (RGB+ED, antialiased, absgrad, viewmat gradient), forward + backward, compared directly."""
    W, H = 1920, 1080
    sc = make_scene(N, seed=0, sh_degree=3 if sh else None)
    vm, K = make_camera(W, H)
    a = {k: v.numpy() for k, v in sc.items()}
    g = torch.Generator().manual_seed(1)
    Gc = torch.randn(1, H, W, 4, generator=g)
    Ga = torch.randn(1, H, W, 1, generator=g)
    P = {k: dev(v).requires_grad_(True) for k, v in sc.items()}
    vmd = dev(vm).requires_grad_(True)
    if sh:
        cam_pos = torch.inverse(vm)[0, :3, 3]
        dirs = a["means"] - cam_pos.numpy()
        rgb_ref = np.clip(oracle.sh_fwd(3, dirs, a["coeffs"]) + 0.5, 0.0, 1.0)
        rgb = torch.clamp(gs.spherical_harmonics(3, P["means"].detach() - dev(cam_pos), P["coeffs"]) + 0.5, 0.0, 1.0)
        np.testing.assert_allclose(rgb.detach().cpu().numpy(), rgb_ref, atol=5e-6)
    else:
        rgb_ref, rgb = a["colors"], P["colors"]
    r_ref, a_ref, m = oracle.rasterization(a["means"], a["quats"], a["scales"], a["opacities"], rgb_ref, vm.numpy(),
                                           K.numpy(), W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    render, alpha, info = gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], rgb, vmd, dev(K), W, H,
                                           packed=False, render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True)
    info["means2d"].retain_grad()
    # ---- integer stages and the projection are bit-exact at full size
    for key in ("radii", "tiles_per_gauss"):
        assert np.array_equal(info[key].cpu().numpy(), m[key]), key
    # gsplat's lists (the default call) bit for bit against the oracle at FULL size, and the opt-in tight lists as ordered
    # sublists of them with a sentinel tail (rerun under mtgs_amd.tight_lists())
    def again():
        with torch.no_grad():
            return gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], rgb.detach(), vmd, dev(K), W, H, packed=False,
                                    render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True)[2]
    assert info.get("n_listed") is None and info["flatten_ids"].numel() == m["flatten_ids"].shape[0]
    assert_tile_lists(info, m, rerun=again)
    for key in ("means2d", "depths", "conics"):
        assert np.array_equal(info[key].detach().cpu().numpy(), m[key]), key
    # ---- structural properties
    ids = listed(info, "isect_ids")
    assert bool((ids[1:] >= ids[:-1]).all()), "isect_ids not sorted"
    off = info["isect_offsets"].flatten()
    assert bool((off[1:] >= off[:-1]).all()) and int(off[-1]) <= ids.numel()
    assert float(alpha.detach().min()) >= 0.0 and float(alpha.detach().max()) < 1.0
    case = f"C{2 if sh else 3} {N // 1000}k 1920x1080 mtgs options"
    flipped = assert_image_close(render.detach().cpu().numpy(), r_ref, m["critical"], name="render", case=case, depth_channel=-1,
                                 alpha=a_ref)
    flipped |= assert_image_close(alpha.detach().cpu().numpy(), a_ref, m["critical"], name="alpha", case=case)
    # ---- backward against the oracle
    from mtgs_amd import wrapper
    dbg = wrapper._debug_rows = {}
    try:
        torch.autograd.backward([render, alpha], [dev(Gc), dev(Ga)])
    finally:
        wrapper._debug_rows = None
    Gc_n, Ga_n = Gc.numpy(), Ga.numpy()
    alc = np.maximum(a_ref, 1e-10)
    Gc_raw = Gc_n.copy()
    Gc_raw[..., -1:] = Gc_n[..., -1:] / alc
    Ga_tot = Ga_n - (m["render_raw"][..., -1:] / alc ** 2) * Gc_n[..., -1:] * (a_ref > 1e-10)
    # ctabs: the same sums of |terms| over the threshold-critical pixels only -- the magnitude bound of the flipped rows
    v2d, vabs, vcon, vcol, vop, tabs, ctabs = oracle.blend_bwd(m["means2d"], m["conics"], m["colors"], m["opacities"], None, W, H, 16,
                                                               m["isect_offsets"], m["flatten_ids"], a_ref, m["last_ids"], Gc_raw,
                                                               Ga_tot, want_term_abs=True, pixel_mask=m["critical"])
    r_vm, r_vq, r_vs, r_vvm = oracle.project_bwd(a["means"], a["quats"], a["scales"], vm.numpy(), K.numpy(), W, H, 0.3,
                                                 m["radii"], m["conics"], m["compensations"], v2d, vcol[..., -1].copy(),
                                                 vcon, vop * a["opacities"][None])
    # ---- every row accounted for.  The rows over 1e-3 relative are (a) sums whose terms cancel (random cotangents), within
    # TERM_REL of their sum of |terms|, or (b) Gaussians on the list of a pixel whose alpha >= 1/255 / T <= 1e-4 decision
    # demonstrably flipped (`flipped`: the critical pixels where the IMAGE differs); nothing else.
    flipped_rows = oracle.gaussians_on_pixels(flipped, m["last_ids"], m["isect_offsets"], m["flatten_ids"], N)
    xy_terms = moment_xy_terms(vabs, tabs, m["conics"], m["opacities"])
    blend_rows_accounted(case, dbg, v2d, vabs, vcon, vcol, vop, tabs, flipped_rows, self_critical=m["critical_gaussians"], crit_terms=ctabs,
                         xy_terms=xy_terms)

    def close(name, got, ref, **kw):
        return assert_grad_close(name, got, ref, case=case, **kw)

    close("means2d.grad", info["means2d"].grad, v2d, term_abs=xy_terms, flipped_rows=flipped_rows, self_critical=m["critical_gaussians"],
          crit_abs=ctabs[0, :, 0:2])
    close("means2d.absgrad", info["means2d"].absgrad, vabs, term_abs=vabs, flipped_rows=flipped_rows, self_critical=m["critical_gaussians"],
          crit_abs=ctabs[0, :, 0:2])
    assert bool((info["means2d"].absgrad >= info["means2d"].grad.abs() - 1e-5).all())
    # behind the projection backward: the VJP itself, applied to the device's own rows, is within 1e-3 on EVERY row
    projection_vjp_accounted(case, oracle, dbg, a, vm.numpy(), K.numpy(), W, H, m, {k: P[k].grad for k in ("means", "quats", "scales", "opacities")})
    close("v_means", P["means"].grad, r_vm)
    close("v_quats", P["quats"].grad, r_vq)
    close("v_scales", P["scales"].grad, r_vs)
    # (the opacity gradient is the sum with the most cancellation under random cotangents -- measured 99.9th percentile
    #  4e-4 at 500k, 1.4e-3 at 2M Gaussians, against <= 6e-4 for every other tensor: its percentile bar is relaxed, but every
    #  row over 1e-3 must be a cancelling sum within TERM_REL of its sum of |terms|, or a flipped row)
    close("v_opacities", P["opacities"].grad, (vop * m["compensations"]).sum(0), row_rel_p999=2.5e-3,
          term_abs=(tabs[..., 3] * m["compensations"]).sum(0), flipped_rows=flipped_rows, self_critical=m["critical_gaussians"],
          crit_abs=(ctabs[..., 5] * m["compensations"]).sum(0))
    close("v_viewmats", vmd.grad[0], r_vvm[0])
    if sh:
        mask = (rgb_ref > 0.0) & (rgb_ref < 1.0)
        ref_vc, _ = oracle.sh_bwd(3, dirs, a["coeffs"], vcol[0, :, :3] * mask)
        close("v_coeffs", P["coeffs"].grad, ref_vc)
    else:
        close("v_colors", P["colors"].grad, vcol[0, :, :3], term_abs=tabs[0, :, 4:7], flipped_rows=flipped_rows, self_critical=m["critical_gaussians"],
              crit_abs=ctabs[0, :, 6:9])


@pytest.mark.parametrize("W,H", [(1280, 720), (960, 540), (333, 211)])
def test_midsize_images_use_more_waves_per_tile(gs, oracle, W, H):
    """Image sizes that select 2 or 4 waves per tile (pick_ppl of blend.hip: fewer than 16000 / 3000 tiles forward,
    6000 / 1536 backward, the four-wave backward with at most 4 channels only; MTGS trains at 960x540): same parity
    bars as the one-wave-per-tile configuration."""
    N = 200_000
    sc = make_scene(N, seed=4)
    vm, K = make_camera(W, H, yaw_deg=30.0)
    a = {k: v.numpy() for k, v in sc.items()}
    g = torch.Generator().manual_seed(2)
    Gc, Ga = torch.randn(1, H, W, 4, generator=g), torch.randn(1, H, W, 1, generator=g)
    r_ref, a_ref, m = oracle.rasterization(a["means"], a["quats"], a["scales"], a["opacities"], a["colors"], vm.numpy(),
                                           K.numpy(), W, H, render_mode="RGB+ED", rasterize_mode="antialiased")
    P = {k: dev(v).requires_grad_(True) for k, v in sc.items()}
    render, alpha, info = gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], dev(vm),
                                           dev(K), W, H, packed=False, render_mode="RGB+ED",
                                           rasterize_mode="antialiased", absgrad=True)
    info["means2d"].retain_grad()

    def again():
        with torch.no_grad():
            return gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], dev(vm), dev(K), W, H, packed=False,
                                    render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True)[2]
    assert_tile_lists(info, m, rerun=again)
    # (these scenes are sparser than C2 / C3: many almost-empty pixels, where expected depth = D / (1 - T) loses relative
    #  precision to the subtraction -- the depth channel's error is larger here than at 1920x1080 for that reason, not because
    #  of the 2- / 4-waves-per-tile kernels: `alpha_at_depth_max_err` and `depth_err_x_alpha` in the parity report)
    case = f"200k {W}x{H}"
    flipped = assert_image_close(render.detach().cpu().numpy(), r_ref, m["critical"], name="render", case=case, depth_channel=-1,
                                 alpha=a_ref)
    flipped |= assert_image_close(alpha.detach().cpu().numpy(), a_ref, m["critical"], name="alpha", case=case)
    from tests.util import REPORT
    rec = [r for r in REPORT if r["kind"] == "image" and r["case"] == case and r["name"] == "render"][-1]
    assert rec["depth_err_x_alpha"] <= 2e-6, rec        # without the 1 / alpha conditioning: fp32 rounding level
    from mtgs_amd import wrapper
    dbg = wrapper._debug_rows = {}
    try:
        torch.autograd.backward([render, alpha], [dev(Gc), dev(Ga)])
    finally:
        wrapper._debug_rows = None
    alc = np.maximum(a_ref, 1e-10)
    Gc_raw = Gc.numpy().copy()
    Gc_raw[..., -1:] = Gc.numpy()[..., -1:] / alc
    Ga_tot = Ga.numpy() - (m["render_raw"][..., -1:] / alc ** 2) * Gc.numpy()[..., -1:] * (a_ref > 1e-10)
    # ctabs: the same sums of |terms| over the threshold-critical pixels only -- the magnitude bound of the flipped rows
    v2d, vabs, vcon, vcol, vop, tabs, ctabs = oracle.blend_bwd(m["means2d"], m["conics"], m["colors"], m["opacities"], None, W, H, 16,
                                                               m["isect_offsets"], m["flatten_ids"], a_ref, m["last_ids"], Gc_raw,
                                                               Ga_tot, want_term_abs=True, pixel_mask=m["critical"])
    flipped_rows = oracle.gaussians_on_pixels(flipped, m["last_ids"], m["isect_offsets"], m["flatten_ids"], N)
    xy_terms = moment_xy_terms(vabs, tabs, m["conics"], m["opacities"])
    blend_rows_accounted(case, dbg, v2d, vabs, vcon, vcol, vop, tabs, flipped_rows, self_critical=m["critical_gaussians"], crit_terms=ctabs,
                         xy_terms=xy_terms)
    for name, got, ref, ta, ca in (("means2d.grad", info["means2d"].grad, v2d, xy_terms, ctabs[0, :, 0:2]),
                                   ("absgrad", info["means2d"].absgrad, vabs, vabs, ctabs[0, :, 0:2]),
                                   ("v_colors", P["colors"].grad, vcol[0, :, :3], tabs[0, :, 4:7], ctabs[0, :, 6:9])):
        assert_grad_close(name, got, ref, case=case, term_abs=ta, flipped_rows=flipped_rows, self_critical=m["critical_gaussians"], crit_abs=ca)


def test_fullsize_properties_linearity_and_determinism(gs):
    """Size-independent properties at configs[2] size: the backward is linear in the cotangent, the
    integer stages are deterministic, culled Gaussians get exactly zero gradient."""
    N, W, H = 2_000_000, 1920, 1080
    sc = make_scene(N, seed=0)
    vm, K = make_camera(W, H)
    P = {k: dev(v).requires_grad_(True) for k, v in sc.items()}
    g = torch.Generator().manual_seed(3)
    G1, G2 = dev(torch.randn(1, H, W, 3, generator=g)), dev(torch.randn(1, H, W, 3, generator=g))

    def run(Gc):
        for p in P.values():
            p.grad = None
        render, alpha, info = gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], dev(vm),
                                               dev(K), W, H, packed=False)
        torch.autograd.backward([render], [Gc])
        return {k: p.grad.clone() for k, p in P.items()}, info, render

    g1, info1, r1 = run(G1)
    g2, info2, r2 = run(G2)
    g12, _, _ = run(G1 + 2.0 * G2)
    assert torch.equal(listed(info1), listed(info2)) and torch.equal(listed(info1, "isect_ids"), listed(info2, "isect_ids"))
    assert torch.equal(r1, r2), "forward is not deterministic"
    for k in P:
        ref = g1[k] + 2.0 * g2[k]
        assert float((g12[k] - ref).abs().max()) <= 2e-3 * float(ref.abs().max()), k
    culled = info1["radii"][0] == 0
    assert float(g1["means"][culled].abs().max()) == 0.0 and float(g1["colors"][culled].abs().max()) == 0.0


@pytest.mark.parametrize("cell", ["MTGS.py", "3DGS.py"])
def test_shipped_option_cell_7_channels_960x540(gs, oracle, cell):
    """The cells the shipped configs drive, at MTGS's training size 960x540 (camera_res_scale_factor 0.5),
    500k Gaussians -- forward and backward against the oracle.
    MTGS.py: RGB + camera-space normals = 6 colour channels + expected depth = 7 blended channels, antialiased, absgrad, viewmat gradient.
    3DGS.py (/root/reference/mtgs/config/3DGS.py:83-95): RGB + expected depth, CLASSIC, absgrad off, camera optimizer off = the pose
    carries no gradient."""
    mtgs = cell == "MTGS.py"
    N, W, H, D = 500_000, 960, 540, (6 if mtgs else 3)
    rmode, absgrad = ("antialiased", True) if mtgs else ("classic", False)
    sc = make_scene(N, seed=5)
    g = torch.Generator().manual_seed(9)
    if mtgs:
        sc["colors"] = torch.cat([sc["colors"], torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)], -1)
    vm, K = make_camera(W, H, yaw_deg=15.0)
    a = {k: v.numpy() for k, v in sc.items()}
    Gc, Ga = torch.randn(1, H, W, D + 1, generator=g), torch.randn(1, H, W, 1, generator=g)
    r_ref, a_ref, m = oracle.rasterization(a["means"], a["quats"], a["scales"], a["opacities"], a["colors"], vm.numpy(),
                                           K.numpy(), W, H, render_mode="RGB+ED", rasterize_mode=rmode)
    P = {k: dev(v).requires_grad_(True) for k, v in sc.items()}
    vmd = dev(vm).requires_grad_(mtgs)
    render, alpha, info = gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], vmd, dev(K), W, H,
                                           packed=False, render_mode="RGB+ED", rasterize_mode=rmode, absgrad=absgrad)
    info["means2d"].retain_grad()
    case = "shipped cell 7ch 500k 960x540" if mtgs else "3DGS.py cell RGB+ED classic 500k 960x540"
    for key in ("radii", "tiles_per_gauss"):
        assert np.array_equal(info[key].cpu().numpy(), m[key]), key

    def again():
        with torch.no_grad():
            return gs.rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], vmd, dev(K), W, H, packed=False,
                                    render_mode="RGB+ED", rasterize_mode=rmode, absgrad=absgrad)[2]
    assert_tile_lists(info, m, rerun=again)
    assert render.shape == (1, H, W, D + 1)
    flipped = assert_image_close(render.detach().cpu().numpy(), r_ref, m["critical"], name="render", case=case, depth_channel=-1,
                                 alpha=a_ref)
    flipped |= assert_image_close(alpha.detach().cpu().numpy(), a_ref, m["critical"], name="alpha", case=case)
    from mtgs_amd import wrapper
    dbg = wrapper._debug_rows = {}
    try:
        torch.autograd.backward([render, alpha], [dev(Gc), dev(Ga)])
    finally:
        wrapper._debug_rows = None
    alc = np.maximum(a_ref, 1e-10)
    Gc_raw = Gc.numpy().copy()
    Gc_raw[..., -1:] = Gc.numpy()[..., -1:] / alc
    Ga_tot = Ga.numpy() - (m["render_raw"][..., -1:] / alc ** 2) * Gc.numpy()[..., -1:] * (a_ref > 1e-10)
    # ctabs: the same sums of |terms| over the threshold-critical pixels only -- the magnitude bound of the flipped rows
    v2d, vabs, vcon, vcol, vop, tabs, ctabs = oracle.blend_bwd(m["means2d"], m["conics"], m["colors"], m["opacities"], None, W, H, 16,
                                                               m["isect_offsets"], m["flatten_ids"], a_ref, m["last_ids"], Gc_raw,
                                                               Ga_tot, want_term_abs=True, pixel_mask=m["critical"])
    comp = m["compensations"] if mtgs else np.ones_like(vop)       # (classic: no compensation factor on the opacity)
    r_vm, r_vq, r_vs, r_vvm = oracle.project_bwd(a["means"], a["quats"], a["scales"], vm.numpy(), K.numpy(), W, H, 0.3,
                                                 m["radii"], m["conics"], m["compensations"], v2d, vcol[..., -1].copy(),
                                                 vcon, vop * a["opacities"][None] if mtgs else None)
    flipped_rows = oracle.gaussians_on_pixels(flipped, m["last_ids"], m["isect_offsets"], m["flatten_ids"], N)
    xy_terms = moment_xy_terms(vabs, tabs, m["conics"], m["opacities"])
    blend_rows_accounted(case, dbg, v2d, vabs, vcon, vcol, vop, tabs, flipped_rows, self_critical=m["critical_gaussians"], crit_terms=ctabs,
                         xy_terms=xy_terms, absgrad=absgrad)
    projection_vjp_accounted(case, oracle, dbg, a, vm.numpy(), K.numpy(), W, H, m, {k: P[k].grad for k in ("means", "quats", "scales", "opacities")})
    fl = dict(flipped_rows=flipped_rows, self_critical=m["critical_gaussians"])
    checks = [("means2d.grad", info["means2d"].grad, v2d, dict(term_abs=xy_terms, crit_abs=ctabs[0, :, 0:2], **fl)),
              ("v_means", P["means"].grad, r_vm, {}), ("v_quats", P["quats"].grad, r_vq, {}),
              ("v_scales", P["scales"].grad, r_vs, {}),
              ("v_opacities", P["opacities"].grad, (vop * comp).sum(0),
               dict(term_abs=(tabs[..., 3] * comp).sum(0), crit_abs=(ctabs[..., 5] * comp).sum(0), **fl)),
              ("v_colors", P["colors"].grad, vcol[0, :, :D], dict(term_abs=tabs[0, :, 4:4 + D], crit_abs=ctabs[0, :, 6:6 + D], **fl))]
    if mtgs:
        checks += [("means2d.absgrad", info["means2d"].absgrad, vabs, dict(term_abs=vabs, crit_abs=ctabs[0, :, 0:2], **fl)),
                   ("v_viewmats", vmd.grad[0], r_vvm[0], {})]
    else:
        assert vmd.grad is None and not hasattr(info["means2d"], "absgrad")
    for name, got, ref, kw in checks:
        assert_grad_close(name, got, ref, case=case, **kw)
