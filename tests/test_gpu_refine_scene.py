"""mtgs_amd.densify.refine_scene (csrc/refine.hip, include/mtgs_refine_scene.h) on the device: refinement_after for every node
of a scene graph in one pass.  Per node it must be refine_gaussians bit for bit (followed by reset_opacities at a reset step);
the gates, the sky node's cull rule and the cull-only phase -- which no call into refine_gaussians can produce -- are compared
with the NumPy restatement tests/refine_scene_refs.py.  The scenes are built once, on the CPU, with every decision away from its
threshold (tests/test_refine_scene_host.py checks that)."""
import warnings
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests import refine_scene_refs as R

pytestmark = pytest.mark.gpu

_cache = {}


def to_node(case, **kw):
    from mtgs_amd.densify import NodeRefine
    dev = torch.device("cuda")
    p, stats, moments, extras, cfg, seed = case[:6]
    up = lambda a: torch.from_numpy(a).to(dev)
    return NodeRefine({k: up(v) for k, v in p.items()}, None if stats is None else tuple(up(s) for s in stats), cfg, seed,
                      moments={k: (up(a), up(b)) for k, (a, b) in moments.items()}, extras={k: up(v) for k, v in extras.items()},
                      cull_rule=case[6] if len(case) > 6 else (100.0, 40.0), **kw)


def identity_nodes():
    """the 120-node scene on the device: read-only, shared by the tests"""
    if "nodes" not in _cache:
        _cache["nodes"] = [to_node(c) for c in R.identity_scene()]
    return _cache["nodes"]


def per_node(step, i, reset=False):
    """refine_gaussians (+ reset_opacities) for node i of the scene at `step`, with the parents mask its hook received; once"""
    from mtgs_amd.densify import refine_gaussians, reset_opacities
    key = (step, i, reset)
    if key not in _cache:
        nd, seen = identity_nodes()[i], []
        new, new_m, info = refine_gaussians(nd.params, nd.stats, nd.cfg, step, nd.seed, moments=nd.moments, extras=nd.extras,
                                            before_rows=seen.append)
        if reset:
            reset_opacities(new["opacities"], nd.cfg, new_m["opacities"])
        _cache[key] = (new, new_m, info, seen[0] if seen else None)
    return _cache[key]


COUNTS = ("n_before", "n_after", "n_old_kept", "n_children", "n_dups", "n_split")


def assert_same(got, want, where):
    """two (new_params, new_moments, info) results, bit for bit"""
    (gp, gm, gi), (wp, wm, wi) = got, want
    assert [int(gi[k]) for k in COUNTS] == [int(wi[k]) for k in COUNTS], (where, [int(gi[k]) for k in COUNTS], [int(wi[k]) for k in COUNTS])
    assert torch.equal(gi["src_index"], wi["src_index"]) and torch.equal(gi["kind"], wi["kind"]), where
    assert gi["src_index"].dtype == torch.int32 and gi["kind"].dtype == torch.uint8
    assert list(gp) == list(wp) and set(gm) == set(wm) and set(gi["extras"]) == set(wi["extras"]), where
    for k in wp:
        assert gp[k].shape == wp[k].shape and gp[k].dtype == wp[k].dtype and torch.equal(gp[k].view(torch.int32), wp[k].view(torch.int32)), (where, k)
        for h in (0, 1):
            assert gm[k][h].shape == wm[k][h].shape and torch.equal(gm[k][h].view(torch.int32), wm[k][h].view(torch.int32)), (where, k, h)
    for k, t in wi["extras"].items():
        assert gi["extras"][k].dtype == t.dtype and torch.equal(gi["extras"][k], t), (where, k)


@pytest.mark.parametrize("step", R.IDENTITY_STEPS)
def test_every_node_equals_refine_gaussians_bit_for_bit(hip_lib, step):
    """120 vanilla-rule nodes (sizes 0, 1, 63, 64, 255, 256, 257, 4000, 20 000 and random ones below 700; plain, multi-colour and
    Fourier nodes; per-node seeds, thresholds, sample counts): every parameter, both moments of each, the extras, src_index, kind,
    every count and the parents masks of the hook.  Steps: before the world-size cull starts, with every rule on, after the
    screen-size rules stop."""
    from mtgs_amd.densify import refine_scene
    nodes, masks = identity_nodes(), []
    out = refine_scene(nodes, step, before_rows=masks.append)
    assert len(out) == len(nodes) == 120 and len(masks) == 1 and len(masks[0]) == 120
    grew = split = culled = 0
    for i, (nd, res) in enumerate(zip(nodes, out)):
        if nd.params["means"].shape[0] == 0:
            assert res is None and masks[0][i] is None
            continue
        want = per_node(step, i)
        assert_same(res, want[:3], (step, i))
        assert masks[0][i].dtype == torch.bool and torch.equal(masks[0][i], want[3]), (step, i)
        assert isinstance(res[2]["n_split"], int)
        grew += res[2]["n_children"] + res[2]["n_dups"]
        split += res[2]["n_split"]
        culled += res[2]["n_before"] - res[2]["n_old_kept"] - res[2]["n_split"]
    assert grew > 2000 and split > 1000 and culled > 200, (grew, split, culled)
    # the results are views of one buffer per tensor name and row shape, not one allocation per node
    plain = [r for r, nd in zip(out, nodes) if r is not None and r[0]["features_rest"].dim() == 3 and r[0]["features_dc"].dim() == 2]
    assert len(plain) > 30 and len({r[0]["features_rest"].untyped_storage().data_ptr() for r in plain}) == 1
    assert len({r[0]["means"].untyped_storage().data_ptr() for r in out if r is not None}) == 1


def test_gates_leave_nodes_untouched_and_the_others_unchanged(hip_lib):
    """Some nodes frozen, some that never collected statistics, some whose config starts densifying later: their result is None,
    their tensors keep their bits, and every other node refines as it does alone."""
    from mtgs_amd.densify import refine_scene
    step = 4000
    base = identity_nodes()
    gated, nodes = {}, []
    for i, nd in enumerate(base):
        why = "frozen" if i % 7 == 3 else "unseen" if i % 7 == 5 else "early" if i % 11 == 7 else None
        if why:
            nd = replace(nd, params={k: v.clone() for k, v in nd.params.items()}, moments={k: (a.clone(), b.clone()) for k, (a, b) in nd.moments.items()},
                         frozen=why == "frozen", stats=None if why == "unseen" else nd.stats,
                         cfg=replace(nd.cfg, densify_from_iter=step) if why == "early" else nd.cfg)
            gated[i] = why
        nodes.append(nd)
    assert {"frozen", "unseen", "early"} == set(gated.values()) and R.IDENTITY_SIZES.index(4000) in gated
    masks = []
    out = refine_scene(nodes, step, before_rows=masks.append)
    for i, (nd, res) in enumerate(zip(nodes, out)):
        if i in gated or nd.params["means"].shape[0] == 0:
            assert res is None and masks[0][i] is None, (i, gated.get(i))
            for k, v in nd.params.items():
                assert torch.equal(v, base[i].params[k]) and torch.equal(nd.moments[k][0], base[i].moments[k][0]), (i, k)
        else:
            assert_same(res, per_node(step, i)[:3], i)


def compare_with_restatement(res, case, step, exact):
    p, stats, moments, extras, cfg, seed, rule = case
    ref, ref_m, masks = R.refinement_after(p, stats, cfg, step, seed, rule, moments=moments)
    new, new_m, info = res
    assert info["n_after"] == int(masks["keep"].sum()) == ref["means"].shape[0]
    assert np.array_equal(info["src_index"].cpu().numpy(), masks["src_index"]) and np.array_equal(info["kind"].cpu().numpy(), masks["kind"])
    assert info["n_split"] == int(masks["splits"].sum()) and info["n_old_kept"] == int((masks["kind"] == 0).sum())
    assert info["n_dups"] == int((masks["kind"] == 1 + cfg.n_split_samples).sum())
    assert info["n_children"] == info["n_after"] - info["n_old_kept"] - info["n_dups"]
    for k in ref:
        got = new[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref[k].shape, k
        if exact:
            assert np.array_equal(got, ref[k]), k                       # rows only leave: every row is a copy
        else:
            tol = 2e-5 if k == "means" else 2e-6                        # (tests/test_gpu_densify.py:103)
            assert np.abs(got - ref[k]).max() <= tol * max(1.0, np.abs(ref[k]).max()), (k, np.abs(got - ref[k]).max())
        for h in (0, 1):
            gm = new_m[k][h].cpu().numpy().astype(np.float64)
            assert np.array_equal(gm, ref_m[k][h].astype(np.float32).astype(np.float64)), (k, h)
    assert np.array_equal(info["extras"]["last"].cpu().numpy(), extras["last"][masks["src_index"]])
    return masks


def test_sky_node_is_culled_by_its_own_rule(hip_lib):
    """A sky node (dome of radius 1000-2000, exp(scale) over 0.05-800) with cull_rule (skybox_radius / 10, skybox_scale_factor)
    = (100, 1000) beside two vanilla nodes, against the restatement: masks, order and counts identical, rows within
    test_gpu_densify.py's tolerances, moments exact.  With (100, 40) -- all refine_gaussians can do -- thousands of these rows go."""
    from mtgs_amd.densify import refine_scene
    cases = R.sky_scene()
    nodes = [to_node(c) for c in cases]
    out = refine_scene(nodes, R.SKY_STEP)
    for res, case in zip(out, cases):
        compare_with_restatement(res, case, R.SKY_STEP, exact=False)
    vanilla = refine_scene([replace(nodes[1], cull_rule=(100.0, 40.0))], R.SKY_STEP)[0]
    assert out[1][2]["n_after"] - vanilla[2]["n_after"] >= 200
    assert float(out[1][0]["scales"].exp().max()) > 40 * 0.5 >= float(vanilla[0]["scales"].exp().max())


def test_cull_only_phase(hip_lib):
    """step >= stop_split_at with continue_cull_post_densification: no row is added, the moments follow their rows, statistics of
    None are accepted where the screen-size rule is off and refused where it is on; equal to the restatement, exactly."""
    from mtgs_amd.densify import refine_scene
    cases = R.cull_only_scene()
    nodes = [to_node(c) for c in cases]
    masks = []
    out = refine_scene(nodes, R.CULL_ONLY_STEP, before_rows=masks.append)
    for res, case, nd, m in zip(out, cases, nodes, masks[0]):
        keep = compare_with_restatement(res, case, R.CULL_ONLY_STEP, exact=True)["keep"]
        info = res[2]
        assert info["n_children"] == info["n_dups"] == info["n_split"] == 0 and 0 < info["n_after"] == info["n_old_kept"] < info["n_before"]
        assert int(info["kind"].max()) == 0 and not bool(m.any())
        assert torch.equal(res[0]["means"], nd.params["means"][torch.from_numpy(keep).cuda()])
    with pytest.raises(ValueError, match="node 1.*max_2Dsize"):
        refine_scene([nodes[0], replace(nodes[2], stats=None)], R.CULL_ONLY_STEP)
    late = replace(nodes[1], cfg=replace(nodes[1].cfg, continue_cull_post_densification=False))
    assert refine_scene([late, nodes[0]], R.CULL_ONLY_STEP)[0] is None


def test_reset_step_equals_refine_then_reset_opacities(hip_lib):
    """step % (reset_alpha_every * refine_every) == refine_every: the clamp of the new opacities and the zeroing of their moments
    happen inside the row move; bit for bit refine_gaussians followed by reset_opacities.  A node whose config resets at another
    step is not touched by its neighbours' reset."""
    from mtgs_amd.densify import refine_gaussians, refine_scene
    step, some = R.RESET_STEP, list(range(0, 40))
    nodes = [identity_nodes()[i] for i in some]
    other = R.IDENTITY_SIZES.index(257)
    nodes[other] = replace(nodes[other], cfg=replace(nodes[other].cfg, reset_alpha_every=7))
    out = refine_scene(nodes, step)
    clamped = 0
    for i, res in zip(some, out):
        if res is None:
            continue
        nd = nodes[i]
        if i == other:
            assert_same(res, refine_gaussians(nd.params, nd.stats, nd.cfg, step, nd.seed, moments=nd.moments, extras=nd.extras), i)
            continue
        want = per_node(step, i, reset=True)
        assert_same(res, want[:3], i)
        cap = float(np.log(2 * nd.cfg.cull_alpha_thresh / (1 - 2 * nd.cfg.cull_alpha_thresh)))
        assert float(res[0]["opacities"].max()) <= np.float32(cap) and not bool(res[1]["opacities"][0].any()) and not bool(res[1]["opacities"][1].any())
        clamped += int((res[0]["opacities"] == np.float32(cap)).sum())
    assert clamped > 5000


@pytest.mark.parametrize("N", [257, 4000])
def test_refine_gaussians_ignores_the_scene_gates(hip_lib, N):
    """refine_gaussians is the one-entry table with the phase forced to densify: with stop_split_at = 100 at step 4000 -- past the
    split phase, where refine_scene leaves the node untouched -- it returns the bits of the same call with the default stop_split_at."""
    from mtgs_amd.densify import refine_gaussians, refine_scene
    step, i = 4000, R.IDENTITY_SIZES.index(N)
    nd = identity_nodes()[i]
    late = replace(nd.cfg, stop_split_at=100)
    assert refine_scene([replace(nd, cfg=late)], step) == [None]
    seen = []
    got = refine_gaussians(nd.params, nd.stats, late, step, nd.seed, moments=nd.moments, extras=nd.extras, before_rows=seen.append)
    want = per_node(step, i)
    assert got[2]["n_before"] == N and got[2]["n_children"] + got[2]["n_dups"] > 0
    assert_same(got, want[:3], N)
    assert len(seen) == 1 and torch.equal(seen[0], want[3])


def test_refine_gaussians_alone_does_not_reset(hip_lib):
    """At the reset step refine_gaussians clamps nothing and zeroes no moment: the reset is reset_opacities, the caller's.  (The
    reset test above applies reset_opacities to its result, which would hide a reset that had already happened.)"""
    from mtgs_amd.densify import refine_gaussians
    step = R.RESET_STEP
    for N in (257, 4000):
        nd = identity_nodes()[R.IDENTITY_SIZES.index(N)]
        new, new_m, info = refine_gaussians(nd.params, nd.stats, nd.cfg, step, nd.seed, moments=nd.moments, extras=nd.extras)
        cap = np.float32(np.log(2 * nd.cfg.cull_alpha_thresh / (1 - 2 * nd.cfg.cull_alpha_thresh)))
        assert float(new["opacities"].max()) > cap
        old = info["kind"] == 0
        src = info["src_index"][old].long()
        assert int(old.sum()) == info["n_old_kept"] > 0
        for h in (0, 1):
            assert torch.equal(new_m["opacities"][h][old].view(torch.int32), nd.moments["opacities"][h][src].view(torch.int32)), (N, h)
        assert torch.equal(new["opacities"][old].view(torch.int32), nd.params["opacities"][src].view(torch.int32)), N


def test_an_empty_node_costs_no_launch_and_no_host_read(hip_lib):
    """N == 0: every tensor is (0, ...), every count 0, and -- under torch.cuda.set_sync_debug_mode("warn") -- no synchronisation
    warning.  Skipped only if the mode does not report a deliberate .item() on this build."""
    from mtgs_amd.densify import refine_gaussians
    nd = identity_nodes()[R.IDENTITY_SIZES.index(0)]
    assert nd.params["means"].shape[0] == 0
    torch.cuda.synchronize()
    prior = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as probe:
            warnings.simplefilter("always")
            torch.ones(1, device="cuda").item()
        if not any("synchroniz" in str(w.message).lower() for w in probe):
            pytest.skip("torch.cuda.set_sync_debug_mode('warn') does not report a deliberate .item() on this build")
        calls = []
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            new, new_m, info = refine_gaussians(nd.params, nd.stats, nd.cfg, 4000, nd.seed, moments=nd.moments, extras=nd.extras,
                                                before_rows=calls.append)
    finally:
        torch.cuda.set_sync_debug_mode(prior)
    assert not [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()] and not calls
    assert [info[k] for k in COUNTS] == [0] * len(COUNTS) and all(isinstance(info[k], int) for k in COUNTS)
    assert info["src_index"].shape == (0,) and info["src_index"].dtype == torch.int32 and info["kind"].shape == (0,) and info["kind"].dtype == torch.uint8
    assert list(new) == list(nd.params) and set(new_m) == set(nd.moments) and set(info["extras"]) == set(nd.extras)
    for k, t in nd.params.items():
        assert new[k].shape == (0,) + tuple(t.shape[1:]) and new[k].dtype == torch.float32 and new[k].is_cuda, k
        assert new_m[k][0].shape == new_m[k][1].shape == new[k].shape, k
    for k, t in nd.extras.items():
        assert info["extras"][k].shape == (0,) + tuple(t.shape[1:]) and info["extras"][k].dtype == t.dtype, k


def test_deterministic_and_independent_of_the_neighbours(hip_lib):
    """Two calls give identical bits; a node's result does not depend on which other nodes are in the scene, or where it stands."""
    from mtgs_amd.densify import refine_scene
    nodes, step = identity_nodes(), 4000
    a, b = refine_scene(nodes, step), refine_scene(nodes, step)
    pick = [i for i in range(len(nodes) - 1, -1, -1) if i % 3 != 1]
    c = refine_scene([nodes[i] for i in pick], step)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert_same(x, y, i)
    for i, z in zip(pick, c):
        assert (z is None) == (a[i] is None)
        if z is not None:
            assert_same(z, a[i], i)
    other = refine_scene([replace(nodes[7], seed=nodes[7].seed + 1)], step)[0]
    assert other[0]["means"].shape != a[7][0]["means"].shape or not torch.equal(other[0]["means"], a[7][0]["means"])     # another seed, other samples


def test_one_host_synchronisation_for_120_nodes(hip_lib):
    """Under torch.cuda.set_sync_debug_mode("warn") the 120-node call raises exactly one synchronisation warning: the read of the
    per-node, per-column survivor totals.  Skipped only if the mode does not report a deliberate .item() on this build."""
    from mtgs_amd.densify import refine_scene
    nodes = identity_nodes()
    refine_scene(nodes, 4000)                              # (the library, the staging buffers and the allocator are warm)
    torch.cuda.synchronize()
    prior = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as probe:
            warnings.simplefilter("always")
            torch.ones(1, device="cuda").item()
        if not any("synchroniz" in str(w.message).lower() for w in probe):
            pytest.skip("torch.cuda.set_sync_debug_mode('warn') does not report a deliberate .item() on this build")
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = refine_scene(nodes, 4000)
    finally:
        torch.cuda.set_sync_debug_mode(prior)
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, syncs
    assert sum(r is not None for r in out) == 119
