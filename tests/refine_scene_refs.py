"""NumPy float64 restatement of refinement_after for ONE node of a scene graph, with everything mtgs_amd.densify.refine_scene
adds to refine_gaussians -- TEST INFRASTRUCTURE ONLY -- and the seeded scenes the host and GPU tests of refine_scene share.

Written from the reference by line number, in the manner of oracle/refine_oracle.py (whose Philox restatement `normals3` and
`quat_to_rotmat` are reused):
  vanilla_gaussian_splatting.py  refinement_after :476-577 (gates :478-484, densify :486-545, cull-only :546-547, opacity reset
                                 :555-573), split_gaussians :630-676, dup_gaussians :678-699, cull_gaussians :579-612,
                                 dup_in_optim :418-437, remove_from_optim :392-410
  skybox_gaussian_splatting.py   cull_gaussians :130-163 -- the same rule with (skybox_radius / 10, skybox_scale_factor) in place
                                 of (100, 40): the rule is the parameter `cull_rule` here
  rigid_node.py :356-366, deformable_node.py :288-298 -- "statistics are None: skip" in the densify phase
"""
from functools import lru_cache

import numpy as np

from mtgs_amd.densify import RefineConfig
from oracle.refine_oracle import normals3, quat_to_rotmat


def refinement_after(params, stats, cfg, step, seed, cull_rule=(100.0, 40.0), moments=None, frozen=False):
    """params: dict of arrays with N rows; stats = (xys_grad_norm, vis_counts, max_2Dsize) or None.  Returns None when the
    reference leaves the node untouched, else (new_params, new_moments | None, masks).  masks: splits, dups (densify phase),
    keep / kind / src_index over the concatenation [old | children | duplicates], `reset`, and `decisions`: a list of
    (name, values, threshold, source row of each value) for EVERY comparison the result depends on -- what a test needs to
    tell how far each decision is from its threshold."""
    N = params["means"].shape[0]
    if frozen:                                                                      # :478
        return None
    if step <= cfg.densify_from_iter:                                               # :480
        return None
    if N <= 0:                                                                      # :483
        return None
    p = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    st = None if stats is None else tuple(np.asarray(t, dtype=np.float64).reshape(-1) for t in stats)
    S = cfg.n_split_samples
    idx = np.arange(N)
    decisions = []
    normals = lambda index, slot: normals3(seed, step, index, slot)
    if step < cfg.stop_split_at:                                                    # :486
        if st is None:                                                              # rigid_node.py:361-364 (a vanilla node asserts, :491)
            return None
        gn, vc, m2 = st
        avg = gn / vc                                                               # :493
        high = avg > cfg.densify_grad_thresh                                        # :498
        decisions.append(("avg_grad", avg, cfg.densify_grad_thresh, idx))
        size = np.exp(p["scales"]).max(-1)
        splits = (size > cfg.densify_size_thresh) & high                            # :500-501
        decisions.append(("size_split", size, cfg.densify_size_thresh, idx))
        if step < cfg.stop_screen_size_at:
            splits |= m2 > cfg.split_screen_size                                    # :503-504
            decisions.append(("screen_split", m2, cfg.split_screen_size, idx))
        sp = idx[splits]
        # split_gaussians (:630-676): sample-major (`.repeat(samps, 1)`)
        z = np.concatenate([normals(sp, s) for s in range(S)], 0) if len(sp) else np.zeros((0, 3))
        rep = lambda a: np.concatenate([a[splits]] * S, 0)
        q = p["quats"][splits] / np.linalg.norm(p["quats"][splits], axis=-1, keepdims=True)
        rots = quat_to_rotmat(np.concatenate([q] * S, 0)) if len(sp) else np.zeros((0, 3, 3))
        split_params = {k: rep(v) for k, v in p.items()}
        split_params["means"] = np.einsum("nij,nj->ni", rots, np.exp(rep(p["scales"])) * z) + rep(p["means"])   # :642-650
        split_params["scales"] = np.log(np.exp(rep(p["scales"])) / 1.6)             # :653
        p["scales"][splits] = np.log(np.exp(p["scales"][splits]) / 1.6)             # :657 (in place)
        size_now = np.exp(p["scales"]).max(-1)
        dups = (size_now <= cfg.densify_size_thresh) & high                         # :509-510
        decisions.append(("size_dup", size_now, cfg.densify_size_thresh, idx))
        dp = idx[dups]
        dup_params = {k: v[dups].copy() for k, v in p.items()}
        if cfg.clone_sample_means and len(dp):                                      # :686-697
            qd = p["quats"][dups] / np.linalg.norm(p["quats"][dups], axis=-1, keepdims=True)
            dup_params["means"] = np.einsum("nij,nj->ni", quat_to_rotmat(qd), np.exp(p["scales"][dups]) * normals(dp, S)) + p["means"][dups]
        allp = {k: np.concatenate([p[k], split_params[k], dup_params[k]], 0) for k in p}   # :512-515
        n_new = len(sp) * S + len(dp)
        m2_all = np.concatenate([m2, np.zeros(n_new)])                              # :517-524
        kind = np.concatenate([np.zeros(N, np.int64)] + [np.full(len(sp), 1 + s) for s in range(S)] + [np.full(len(dp), 1 + S)])
        src = np.concatenate([idx] + [sp] * S + [dp])
        extra = np.concatenate([splits, np.zeros(n_new, bool)])                     # :534-543
    elif cfg.continue_cull_post_densification:                                      # :546-547
        splits = dups = np.zeros(N, bool)
        allp, n_new, kind, src, extra = p, 0, np.zeros(N, np.int64), idx, None
        m2_all = None if st is None else st[2]
    else:                                                                           # :548-550: nothing is pruned (and no reset: :555 needs step < stop_split_at)
        return None
    # cull_gaussians (:579-612; skybox_gaussian_splatting.py:130-163 with its own constants)
    alpha = 1.0 / (1.0 + np.exp(-allp["opacities"].reshape(-1)))
    culls = alpha < cfg.cull_alpha_thresh                                           # :586
    decisions.append(("alpha", alpha, cfg.cull_alpha_thresh, src))
    if extra is not None:
        culls = culls | extra                                                       # :592
    if step > cfg.refine_every * cfg.reset_alpha_every:                             # :595
        radius, factor = cull_rule
        norm = np.linalg.norm(allp["means"], axis=-1)
        far = norm > radius                                                         # :599 / sky :147
        thresh = np.where(far, factor, 1.0) * cfg.cull_scale_thresh                 # :600 / sky :148
        size_all = np.exp(allp["scales"]).max(-1)
        toobig = size_all > thresh                                                  # :603
        decisions += [("norm", norm, radius, src), ("size_cull_near", size_all, cfg.cull_scale_thresh, src),
                      ("size_cull_far", size_all, factor * cfg.cull_scale_thresh, src)]
        if step < cfg.stop_screen_size_at:
            if m2_all is None:
                raise ValueError("max_2Dsize is None and the screen-size rule is on")          # the assert of :607
            toobig = toobig | (m2_all > cfg.cull_screen_size)                       # :608-610
            decisions.append(("screen_cull", m2_all, cfg.cull_screen_size, src))
        culls = culls | toobig                                                      # :612
    keep = ~culls
    new = {k: v[keep] for k, v in allp.items()}
    new_m = None
    if moments is not None:                                                         # dup_in_optim: zeros (:418-437); remove_from_optim (:392-410)
        new_m = {}
        for k, (a, b) in moments.items():
            pad = lambda t: np.concatenate([np.asarray(t, np.float64), np.zeros((n_new,) + t.shape[1:])], 0)[keep]
            new_m[k] = (pad(a), pad(b))
    reset = step < cfg.stop_split_at and step % (cfg.reset_alpha_every * cfg.refine_every) == cfg.refine_every   # :555
    if reset:
        v = cfg.cull_alpha_thresh * 2.0                                             # :559
        new["opacities"] = np.minimum(new["opacities"], np.log(v / (1.0 - v)))      # :560-563
        if new_m is not None and "opacities" in new_m:                              # :565-573
            new_m["opacities"] = tuple(np.zeros_like(t) for t in new_m["opacities"])
    return new, new_m, {"splits": splits, "dups": dups, "keep": keep, "kind": kind[keep], "src_index": src[keep], "reset": reset,
                        "decisions": decisions}


def margins(result):
    """{decision name: smallest |value - threshold| / |threshold|} of one restatement result"""
    out = {}
    for name, v, t, _ in result[2]["decisions"]:
        out[name] = min(out.get(name, np.inf), float(np.min(np.abs(v - t) / abs(t))) if len(v) else np.inf)
    return out


def near_rows(result, N, rel):
    """bool [N]: source rows with a decision within `rel` (relative) of its threshold"""
    bad = np.zeros(N, bool)
    for _, v, t, src in result[2]["decisions"]:
        bad[src[np.abs(v - t) <= rel * abs(t)]] = True
    return bad


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-3          # no decision of a shared scene is closer to its threshold than this (relative)
KINDS = ("plain", "multi", "fourier")


def raw_node(N, seed, kind="plain", sky=False):
    """float32 inputs of one node in the value ranges of tests/test_gpu_densify.py::_refine_case; sky: means on and inside a dome
    of radius 1000-2000, exp(scale) log-uniform over 0.05-800."""
    g = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if sky:
        d = g.standard_normal((N, 3))
        d[:, 1] = np.abs(d[:, 1])
        means = d / np.linalg.norm(d, axis=-1, keepdims=True) * g.uniform(1000.0, 2000.0, (N, 1))
        scales = np.log(0.05) + g.random((N, 3)) * (np.log(800.0) - np.log(0.05))
    else:
        means = (g.random((N, 3)) * 2 - 1) * np.array([60.0, 8.0, 140.0])
        scales = np.log(g.random((N, 3)) * 0.6 + 0.01)
    p = {"means": f(means), "scales": f(scales), "quats": f(g.standard_normal((N, 4)) * 1.7), "opacities": f(g.standard_normal((N, 1)) * 3.0)}
    if kind == "fourier":
        p["features_dc"] = f(g.standard_normal((N, 5, 3)))
        p["features_rest"] = f(g.standard_normal((N, 15, 3)))
    elif kind == "multi":
        p["features_dc"] = f(g.standard_normal((N, 3)))
        p["features_rest"] = f(g.standard_normal((N, 3, 15, 3)))
        p["features_adapters"] = f(g.standard_normal((N, 3, 3)))
    else:
        p["features_dc"] = f(g.standard_normal((N, 3)))
        p["features_rest"] = f(g.standard_normal((N, 15, 3)))
    stats = (f(g.random(N) * 0.028), f(g.integers(1, 12, N)), f(g.random(N) * 180.0))
    moments = {k: (f(g.standard_normal(v.shape)), f(g.random(v.shape))) for k, v in p.items()}
    extras = {"last": g.integers(0, 1 << 30, (N,)).astype(np.int32)}
    return p, stats, moments, extras


def clean_node(N, seed, cfgs_steps, node_seed, kind="plain", sky=False, cull_rule=(100.0, 40.0)):
    """raw_node with every row that has a decision within 2 * MARGIN of its threshold -- under any (cfg, step, stats or None)
    of `cfgs_steps` -- drawn again (geometry and statistics of that row from another seed) until none is left: the seeds are
    chosen here, on the CPU."""
    p, stats, moments, extras = raw_node(N, seed, kind, sky)
    for attempt in range(1, 40):
        bad = np.zeros(N, bool)
        for cfg, step, with_stats in cfgs_steps:
            r = refinement_after(p, stats if with_stats else None, cfg, step, node_seed, cull_rule)
            if r is not None:
                bad |= near_rows(r, N, 2 * MARGIN)
        if not bad.any():
            return p, stats, moments, extras
        p2, stats2, _, _ = raw_node(N, seed + 7919 * attempt, kind, sky)
        for k in ("means", "scales", "quats", "opacities"):
            p[k][bad] = p2[k][bad]
        for a, b in zip(stats, stats2):
            a[bad] = b[bad]
    raise AssertionError("no clean draw")


IDENTITY_STEPS = (500, 4000, 16000)
RESET_STEP = 3100                    # 3100 % (30 * 100) == 100 == refine_every
IDENTITY_SIZES = (0, 1, 63, 64, 255, 256, 257, 4000, 20000)


def identity_cfg(i):
    """Per-node control config: thresholds, sample count and clone_sample_means vary; stop_split_at raised as in test_gpu_densify.py"""
    return RefineConfig(stop_split_at=20000, densify_from_iter=0, n_split_samples=(2, 3, 1, 2, 4)[i % 5], clone_sample_means=i % 3 != 1,
                        densify_grad_thresh=0.001 * (1 + 0.1 * (i % 4)), densify_size_thresh=0.2 + 0.02 * (i % 3),
                        cull_alpha_thresh=0.005 + 0.001 * (i % 2))


@lru_cache(maxsize=None)
def identity_scene():
    """120 vanilla-rule nodes: the sizes at which the kernels' blocks begin and end, random sizes below 700, one node of 20 000;
    plain, multi-colour (T = 3) and Fourier nodes in turn; seeds and configs differ per node.  [(params, stats, moments, extras,
    cfg, seed)]"""
    g = np.random.default_rng(2024)
    sizes = list(IDENTITY_SIZES) + [int(x) for x in g.integers(1, 700, 120 - len(IDENTITY_SIZES))]
    out = []
    for i, N in enumerate(sizes):
        cfg, seed = identity_cfg(i), 1234567 + 104729 * i + (i << 40)
        steps = [(cfg, s, True) for s in IDENTITY_STEPS + (RESET_STEP,)]
        out.append(clean_node(N, 100 + i, steps, seed, KINDS[i % 3]) + (cfg, seed))
    return out


SKY_RULE = (100.0, 1000.0)           # skybox_radius 1000 / 10, skybox_scale_factor 1000 (the shipped values)
SKY_STEP = 4000


@lru_cache(maxsize=None)
def sky_scene():
    """A sky node beside two vanilla nodes.  [(params, stats, moments, extras, cfg, seed, cull_rule)]"""
    cfg = RefineConfig(stop_split_at=20000, densify_from_iter=0)
    steps = [(cfg, SKY_STEP, True)]
    return [clean_node(3000, 11, steps, 501, "plain") + (cfg, 501, (100.0, 40.0)),
            clean_node(6000, 12, steps, 502, "multi", sky=True, cull_rule=SKY_RULE) + (cfg, 502, SKY_RULE),
            clean_node(1500, 13, steps, 503, "fourier") + (cfg, 503, (100.0, 40.0))]


CULL_ONLY_STEP = 16000


@lru_cache(maxsize=None)
def cull_only_scene():
    """Past stop_split_at with continue_cull_post_densification.  Node 0: the screen-size rule is off, statistics None; node 1: the
    same with statistics given (they are not read); node 2: stop_screen_size_at raised, so the screen-size rule reads max_2Dsize;
    node 3: the sky rule.  [(params, stats | None, moments, extras, cfg, seed, cull_rule)]"""
    off = RefineConfig(continue_cull_post_densification=True, densify_from_iter=0)
    on = RefineConfig(continue_cull_post_densification=True, densify_from_iter=0, stop_screen_size_at=20000)
    out = []
    for i, (N, cfg, with_stats, kind, sky, rule) in enumerate([(3000, off, False, "plain", False, (100.0, 40.0)), (700, off, True, "multi", False, (100.0, 40.0)),
                                                            (2500, on, True, "fourier", False, (100.0, 40.0)), (2000, off, False, "plain", True, SKY_RULE)]):
        p, stats, moments, extras = clean_node(N, 40 + i, [(cfg, CULL_ONLY_STEP, with_stats)], 900 + i, kind, sky, rule)
        out.append((p, stats if with_stats else None, moments, extras, cfg, 900 + i, rule))
    return out
