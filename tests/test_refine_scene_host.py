"""mtgs_amd.densify.refine_scene without a GPU: the NumPy restatement it is tested against (tests/refine_scene_refs.py) agrees
with oracle/refine_oracle.py where the two overlap, the seeded scenes of tests/test_gpu_refine_scene.py keep every decision away
from its threshold, the sky case separates the two cull rules, the C entry points of include/mtgs_refine_scene.h are declared,
bound, exported and refuse bad arguments by name, and refine_scene refuses what it does not support before it touches a device."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import refine_scene_refs as R

ROOT = Path(__file__).resolve().parents[1]
ALL_DECISIONS = {"avg_grad", "size_split", "size_dup", "screen_split", "alpha", "norm", "size_cull_near", "size_cull_far", "screen_cull"}


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step, clone, kind", [(500, True, "plain"), (4000, True, "plain"), (4000, False, "multi"), (16000, True, "fourier")])
def test_restatement_equals_the_oracle_in_the_densify_phase(step, clone, kind):
    """Rule (100, 40), step < stop_split_at: exactly oracle.refine_oracle.refinement_after, array for array."""
    from mtgs_amd.densify import RefineConfig
    from oracle import refine_oracle as ro
    cfg = RefineConfig(clone_sample_means=clone, stop_split_at=20000, densify_from_iter=0)
    seed = 1234567 + (7 << 33)
    p, stats, moments, _ = R.raw_node(5000, step, kind)
    want, want_m, wm = ro.refinement_after(p, stats, cfg, step, lambda idx, slot: ro.normals3(seed, step, idx, slot), moments=moments)
    got, got_m, gm = R.refinement_after(p, stats, cfg, step, seed, (100.0, 40.0), moments=moments)
    assert wm["splits"].sum() > 50 and wm["dups"].sum() > 50 and (~wm["keep"]).sum() > 50
    for k in ("splits", "dups", "keep", "kind", "src_index"):
        assert np.array_equal(gm[k], wm[k]), k
    assert not gm["reset"] and set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got_m[k][0], want_m[k][0]) and np.array_equal(got_m[k][1], want_m[k][1]), k


def test_restatement_gates_and_reset():
    from dataclasses import replace
    from mtgs_amd.densify import RefineConfig
    cfg = RefineConfig(densify_from_iter=500)
    p, stats, moments, _ = R.raw_node(800, 5)
    run = lambda cfg=cfg, step=4000, stats=stats, **kw: R.refinement_after(p, stats, cfg, step, 9, moments=moments, **kw)
    assert run(frozen=True) is None and run(step=500) is None and run(step=501) is not None           # :478, :480
    assert run(stats=None) is None                                                                     # rigid_node.py:361-364
    assert R.refinement_after({k: v[:0] for k, v in p.items()}, tuple(s[:0] for s in stats), cfg, 4000, 9) is None   # :483
    assert run(step=15000) is None                                                                     # :548-550
    late = replace(cfg, continue_cull_post_densification=True)
    new, new_m, m = run(cfg=late, step=15000, stats=None)                                              # :546-547: rows only leave
    assert m["keep"].shape == (800,) and 0 < m["keep"].sum() < 800 and np.array_equal(m["src_index"], np.flatnonzero(m["keep"]))
    assert np.array_equal(new["features_rest"], p["features_rest"][m["keep"]])
    assert np.array_equal(new_m["quats"][1], moments["quats"][1][m["keep"]])
    with pytest.raises(ValueError, match="max_2Dsize"):                                                # the assert of :607
        run(cfg=replace(late, stop_screen_size_at=20000), step=15000, stats=None)
    # the reset: step % (30 * 100) == 100, before stop_split_at only
    new, new_m, m = run(step=3100)
    plain, plain_m, pm = run(step=3100, cfg=replace(cfg, reset_alpha_every=7))
    cap = np.log(0.01 / 0.99)
    assert m["reset"] and not pm["reset"] and np.array_equal(m["keep"], pm["keep"])
    assert new["opacities"].max() == cap and plain["opacities"].max() > cap
    assert np.array_equal(new["opacities"], np.minimum(plain["opacities"], cap))
    assert not new_m["opacities"][0].any() and not new_m["opacities"][1].any() and plain_m["opacities"][1].any()
    assert np.array_equal(new_m["means"][0], plain_m["means"][0])


# ---- the seeded scenes of the GPU tests ------------------------------------------------------------------------------------------
def scene_margins(nodes, steps):
    """smallest relative distance per decision over a scene, and the decisions that occurred"""
    worst = {}
    for node in nodes:
        p, stats, _, _, cfg, seed = node[:6]
        rule = node[6] if len(node) > 6 else (100.0, 40.0)
        for step in steps:
            r = R.refinement_after(p, stats, cfg, step, seed, rule)
            if r is not None:
                for k, v in R.margins(r).items():
                    worst[k] = min(worst.get(k, np.inf), v)
    return worst


def test_no_decision_of_the_gpu_scenes_is_near_its_threshold():
    """norm against the radius, max exp(scale) against the densify threshold (before and after the shrink) and both cull thresholds,
    sigmoid(opacity), the average gradient and both screen sizes: all of them occur, none within MARGIN (relative)."""
    seen = {}
    for name, nodes, steps in (("identity", R.identity_scene(), R.IDENTITY_STEPS + (R.RESET_STEP,)), ("sky", R.sky_scene(), (R.SKY_STEP,)),
                               ("cull-only", R.cull_only_scene(), (R.CULL_ONLY_STEP,))):
        worst = scene_margins(nodes, steps)
        print(name, {k: f"{v:.2e}" for k, v in sorted(worst.items())})
        assert all(v > R.MARGIN for v in worst.values()), (name, worst)
        seen[name] = set(worst)
    assert seen["identity"] == ALL_DECISIONS and seen["sky"] == ALL_DECISIONS
    assert seen["cull-only"] == {"alpha", "norm", "size_cull_near", "size_cull_far", "screen_cull"}
    sizes = [n[0]["means"].shape[0] for n in R.identity_scene()]
    assert len(sizes) == 120 and sizes[:9] == list(R.IDENTITY_SIZES) and max(sizes[9:]) < 700
    assert len({n[5] for n in R.identity_scene()}) == 120 and len({repr(n[4]) for n in R.identity_scene()}) > 20


def test_the_sky_case_separates_the_two_rules():
    """The sky node holds Gaussians the sky rule keeps and (100, 40) would cull -- at least 200 -- and Gaussians both cull."""
    p, stats, moments, _, cfg, seed, rule = R.sky_scene()[1]
    assert rule == R.SKY_RULE == (100.0, 1000.0)
    norm, size = np.linalg.norm(p["means"].astype(np.float64), axis=-1), np.exp(p["scales"].astype(np.float64)).max(-1)
    assert 1000.0 <= norm.min() and norm.max() <= 2000.0 + 1e-3 and p["means"][:, 1].min() >= 0
    assert size.min() < 1.0 and size.max() > 700.0
    sky = R.refinement_after(p, stats, cfg, R.SKY_STEP, seed, rule)[2]
    van = R.refinement_after(p, stats, cfg, R.SKY_STEP, seed, (100.0, 40.0))[2]
    assert np.array_equal(sky["splits"], van["splits"]) and sky["keep"].shape == van["keep"].shape
    only_sky = sky["keep"] & ~van["keep"]
    both_cull = ~sky["keep"] & ~van["keep"] & ~np.concatenate([sky["splits"], np.zeros(len(sky["keep"]) - len(sky["splits"]), bool)])
    print(f"kept by the sky rule only: {int(only_sky.sum())}; culled by both: {int(both_cull.sum())}; kept by both: {int((sky['keep'] & van['keep']).sum())}")
    assert only_sky.sum() >= 200 and both_cull.sum() >= 200 and not (van["keep"] & ~sky["keep"]).any()
    assert only_sky[:len(sky["splits"])].sum() >= 50 and only_sky[len(sky["splits"]):].sum() >= 50     # old rows and new ones


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NAMES = ["mtgs_refine_scene_apply", "mtgs_refine_scene_classify", "mtgs_refine_scene_rows", "mtgs_refine_scene_table_bytes"]


def test_the_header_is_declared_bound_and_exported(hip_lib):
    """include/mtgs_refine_scene.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed
    record tests/golden/abi_signatures_refine_scene.txt and the library): its entry points, its two tables and its constants."""
    from mtgs_amd import _abi, _lib, densify
    abi = _abi.header_abi("mtgs_refine_scene.h")
    assert sorted(_lib.GROUPS["mtgs_refine_scene.h"]) == NAMES
    # the two tables: the record dtypes the Python layer uploads are the header's structs, of the size the library reports
    nb, mb = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.mtgs_refine_scene_table_bytes(C.byref(nb), C.byref(mb)) == 0
    assert (nb.value, mb.value) == (densify._REFINE_NODE.itemsize, densify._REFINE_MOVE.itemsize) == (264, 64)
    assert densify._REFINE_NODE == abi.structs["mtgs_refine_node"] and densify._REFINE_MOVE == abi.structs["mtgs_refine_move"]
    assert abi.constants["MTGS_REFINE_MAX_COLUMNS"] == 6 and (abi.constants["MTGS_REFINE_DENSIFY"], abi.constants["MTGS_REFINE_CULL_ONLY"]) == (1, 2)


def test_the_c_compiler_lays_the_tables_out_as_the_reader_does(tmp_path):
    import shutil
    import subprocess
    from mtgs_amd import _abi
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    abi = _abi.header_abi("mtgs_refine_scene.h")
    prints = []
    for name, dtype in abi.structs.items():
        prints.append(f'printf("{name} . %zu 0\\n", sizeof({name}));')
        prints += [f'printf("{name} {f} %zu %zu\\n", sizeof((({name} *)0)->{f}), offsetof({name}, {f}));' for f in dtype.names]
    src = tmp_path / "h.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mtgs_refine_scene.h"\nint main(void) {\n' + "\n".join(prints) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "h")])
    for line in subprocess.check_output([str(tmp_path / "h")], text=True).splitlines():
        name, field, size, offset = line.split()
        dtype = abi.structs[name]
        want = (dtype.itemsize, 0) if field == "." else (dtype.fields[field][0].itemsize, dtype.fields[field][1])
        assert (int(size), int(offset)) == want, line


def test_host_side_argument_checks(hip_lib):
    """Every refusal happens before a launch and names the argument (no device is needed: the pointers are never followed)."""
    err = lambda: hip_lib.mtgs_rast_last_error().decode()
    buf = (C.c_int64 * 8)()
    a = C.addressof(buf)
    n = C.c_size_t(0)
    assert hip_lib.mtgs_refine_scene_table_bytes(None, C.byref(n)) == 1 and "null pointer: node_bytes" in err()
    assert hip_lib.mtgs_refine_scene_table_bytes(C.byref(n), None) == 1 and "null pointer: move_bytes" in err()
    classify = lambda n_nodes=2, table=a, blocks=3, n_total=600, ncol=4, counts=a, flags=a, parents=None: \
        hip_lib.mtgs_refine_scene_classify(n_nodes, table, blocks, n_total, ncol, 4000, counts, flags, parents, None)
    assert classify(n_nodes=-1) == 1 and "n_nodes < 0 (-1)" in err()
    assert classify(n_total=1 << 31) == 1 and "n_total outside [0, 2^31)" in err()
    assert classify(n_total=-5) == 1 and "n_total outside" in err()
    for bad in (2, 7):
        assert classify(ncol=bad) == 4 and f"n_columns outside [3, 6] ({bad})" in err()
    assert classify(blocks=601) == 1 and "total_blocks outside [0, n_total] (601)" in err()
    for kw, word in (({"table": None}, "table"), ({"counts": None}, "counts"), ({"flags": None}, "flags")):
        assert classify(**kw) == 1 and f"mtgs_refine_scene_classify: null pointer: {word}" in err(), kw
    assert classify(table=a + 4) == 1 and "table must be 8-byte aligned" in err()
    assert classify(n_nodes=0, table=None, counts=None, flags=None) == 0                  # no node: a no-op
    assert classify(n_total=0, blocks=0, table=None) == 0                                 # an all-empty scene
    apply = lambda n_nodes=2, table=a, blocks=3, out_blocks=4, n_total=600, n_out=900, ncol=4, flags=a, incl=a, src=a, kind=a, om=a, os=a: \
        hip_lib.mtgs_refine_scene_apply(n_nodes, table, blocks, out_blocks, n_total, n_out, ncol, 4000, flags, incl, src, kind, om, os, None)
    assert apply(n_nodes=-2) == 1 and "n_nodes < 0" in err()
    assert apply(n_out=1 << 31) == 1 and "n_out_total outside [0, 2^31)" in err()
    assert apply(n_total=1 << 31) == 1 and "n_total outside" in err()
    assert apply(ncol=9) == 4 and "n_columns outside [3, 6] (9)" in err()
    assert apply(out_blocks=901) == 1 and "out_blocks outside [0, n_out_total] (901)" in err()
    assert apply(blocks=-1) == 1 and "total_blocks outside" in err()
    for kw, word in (({"table": None}, "table"), ({"flags": None}, "flags"), ({"incl": None}, "incl"), ({"src": None}, "src_index"),
                     ({"kind": None}, "kind"), ({"om": None}, "out_means"), ({"os": None}, "out_scales")):
        assert apply(**kw) == 1 and f"mtgs_refine_scene_apply: null pointer: {word}" in err(), kw
    assert apply(n_out=0, out_blocks=0, src=None, kind=None, om=None, os=None) == 0       # every Gaussian culled
    assert apply(n_nodes=0, table=None) == 0
    rows = lambda n_moves=3, moves=a, blocks=5, src=a, kind=a: hip_lib.mtgs_refine_scene_rows(n_moves, moves, blocks, src, kind, None)
    assert rows(n_moves=-1) == 1 and "n_moves < 0 (-1)" in err()
    assert rows(blocks=1 << 31) == 1 and "total_blocks outside [0, 2^31)" in err()
    for kw, word in (({"moves": None}, "moves"), ({"src": None}, "src_index"), ({"kind": None}, "kind")):
        assert rows(**kw) == 1 and f"mtgs_refine_scene_rows: null pointer: {word}" in err(), kw
    assert rows(moves=a + 4) == 1 and "moves must be 8-byte aligned" in err()
    assert rows(n_moves=0, moves=None) == 0 and rows(blocks=0, src=None, kind=None) == 0


# ---- refine_scene: what it refuses and what it decides on the host -----------------------------------------------------------------
def _cpu_node(N=4, **kw):
    from mtgs_amd.densify import NodeRefine, RefineConfig
    p = {"means": torch.zeros(N, 3), "scales": torch.zeros(N, 3), "quats": torch.ones(N, 4), "opacities": torch.zeros(N, 1)}
    return NodeRefine(p, (torch.ones(N), torch.ones(N), torch.ones(N)), kw.pop("cfg", RefineConfig()), 1, **kw)


def test_refine_scene_refuses_cpu_tensors_and_isotropic_nodes():
    import mtgs_amd
    from mtgs_amd.densify import refine_scene
    assert mtgs_amd.refine_scene is refine_scene and {"refine_scene", "NodeRefine", "RefineConfig"} <= set(mtgs_amd.__all__)
    with pytest.raises(RuntimeError, match="HIP device"):
        refine_scene([_cpu_node()], 4000)
    with pytest.raises(RuntimeError, match="HIP device"):          # also when the node would stay untouched
        refine_scene([_cpu_node(frozen=True)], 4000)
    iso = _cpu_node()
    iso.params["scales"] = torch.zeros(4, 1)
    del iso.params["quats"]
    with pytest.raises(NotImplementedError, match=r"node 1 is isotropic.*\(4, 1\).*no quats"):
        refine_scene([_cpu_node(), iso], 4000)
    assert refine_scene([], 4000) == []


def test_refine_phase_follows_the_gates():
    from dataclasses import replace
    from mtgs_amd.densify import RefineConfig, refine_phase
    cfg = RefineConfig()
    assert cfg.densify_from_iter == 500 and list(vars(cfg))[-1] == "densify_from_iter"
    assert refine_phase(_cpu_node(), 4000) == 1 and refine_phase(_cpu_node(), 14999) == 1
    assert refine_phase(_cpu_node(frozen=True), 4000) == 0 and refine_phase(_cpu_node(), 500) == 0 and refine_phase(_cpu_node(), 501) == 1
    assert refine_phase(_cpu_node(N=0), 4000) == 0
    unseen = _cpu_node()
    unseen.stats = None
    assert refine_phase(unseen, 4000) == 0
    assert refine_phase(_cpu_node(), 15000) == 0
    late = replace(cfg, continue_cull_post_densification=True)
    assert refine_phase(_cpu_node(cfg=late), 15000) == 2 and refine_phase(_cpu_node(cfg=late), 14999) == 1
    unseen.cfg = late
    assert refine_phase(unseen, 15000) == 2 and refine_phase(unseen, 14999) == 0
