"""tests/project_refs.py without a GPU: the per-pair derivatives equal float64 central differences of the float64 forward (clamped
Gaussians included), the scenes contain the edges they promise, and the fp32 C oracle (oracle/gsplat_oracle.c: fp32, contraction off,
gsplat's evaluation order) lies within the constants stored in project_refs -- the numbers tests/test_gpu_project_edges.py derives its
bounds from.  Nothing here runs a HIP kernel."""
import numpy as np
import pytest

from tests import project_refs as R

# (antialiased, v_compensations, v_opac_eff): every combination the entry point accepts
OPTIONS = [(True, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True), (False, False, False)]


def _outputs(means, quats, scales, vm, K):
    f = R.forward(means, quats, scales, vm, K)
    return np.concatenate([f["means2d"], f["depths"][..., None], f["conics"], f["comp"][..., None]], axis=-1)      # [C, n, 7]


@pytest.mark.parametrize("name", ["c3-n257", "c1-n600"])
def test_derivatives_are_central_differences(name):
    """Gaussians 0 .. 12 (one of every clamp group and seven unclamped ones) in the first and the last camera: every derivative of
    every output with respect to mean, quaternion, scale and the camera's 12 entries, 1e-6 of the largest of its group."""
    sc = R.scene(name)
    sel = np.arange(13)
    for cam in sorted({0, sc.C - 1}):
        d = R.derivatives(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, np.full(sel.size, cam), sel)
        scale = d["comp"] / (d["comp"] + R.COMP_EPS)
        base = [np.array(v[sel] if k < 3 else v[cam:cam + 1], dtype=np.float64)
                for k, v in enumerate((sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks))]
        for which, key in enumerate(("means", "quats", "scales", "viewmat")):
            an = d[key].copy()
            an[:, 6] /= scale.reshape((-1,) + (1,) * (an.ndim - 2))
            arr = base[which]
            fd = np.zeros_like(an)
            comps = [(i, j) for i in range(3) for j in range(4)] if key == "viewmat" else [(k,) for k in range(arr.shape[1])]
            for comp in comps:
                vals = []
                for sgn in (1, -1):
                    p = [a.copy() for a in base]
                    h = 1e-6
                    if key == "viewmat":
                        p[3][0][comp] += sgn * h
                    else:
                        p[which][:, comp[0]] += sgn * h
                    vals.append(_outputs(*p)[0])
                fd[(slice(None), slice(None)) + comp] = (vals[0] - vals[1]) / 2e-6
            if key == "viewmat":
                assert not an[..., 3, :].any()
            for j in range(7):
                err = np.abs(fd[:, j] - an[:, j]).max() / max(np.abs(an[:, j]).max(), 1e-30)
                assert err <= 1e-6, (name, cam, key, R.COMPONENTS[j], err)


@pytest.mark.parametrize("name", R.SCENES)
def test_scene_contains_its_edges(name):
    sc = R.scene(name)
    m64 = sc.means.astype(np.float64)
    side_count = {k: 0 for k in ("x+", "x-", "y+", "y-", "xy")}
    for c in range(sc.C):
        vm = sc.viewmats[c].astype(np.float64)
        cam = m64 @ vm[:3, :3].T + vm[:3, 3]
        assert cam[:, 2].min() >= 1.5 and cam[:, 2].max() <= 11.0, "depth far inside the near plane"
        lxp, lxn, lyp, lyn = R.limits(sc.Ks[c].astype(np.float64))
        xz, yz = cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2]
        for v, lim in ((xz, lxp), (-xz, lxn), (yz, lyp), (-yz, lyn)):
            assert np.abs(v - lim).min() > 1e-3, "nothing on a clamp limit: torch.minimum splits the gradient at a tie"
        cx, cy = (xz > lxp) | (xz < -lxn), (yz > lyp) | (yz < -lyn)
        # the groups clamp in EVERY camera as they were built for the first
        g = sc.group
        assert (xz[g == 0] > lxp).all() and (xz[g == 1] < -lxn).all() and (yz[g == 2] > lyp).all() and (yz[g == 3] < -lyn).all()
        assert (cx & cy)[(g == 4) | (g == 5)].all() and not (cx | cy)[g < 0].any()
        side_count["x+"] += int((xz > lxp).sum()); side_count["x-"] += int((xz < -lxn).sum())
        side_count["y+"] += int((yz > lyp).sum()); side_count["y-"] += int((yz < -lyn).sum())
        side_count["xy"] += int((cx & cy).sum())
    if sc.N >= 12:
        k = sc.C * (sc.N // 12)
        assert side_count["x+"] >= 2 * k and side_count["x-"] >= 2 * k and side_count["y+"] >= 2 * k and side_count["y-"] >= 2 * k
        assert side_count["xy"] >= 2 * k
    norm = np.linalg.norm(sc.quats.astype(np.float64), axis=1)
    assert norm.min() >= 0.19 and norm.max() <= 5.1 and (sc.N < 50 or (norm.min() < 0.5 and norm.max() > 3.0)), "norms far from 1, none near 0"
    ratio = sc.scales.max(axis=1) / sc.scales.min(axis=1)
    assert ratio.max() <= 6.01 and sc.scales.min() >= 0.029
    f = R.scene_forward(name)
    assert np.isfinite(f["conics"]).all() and f["comp"].min() > 0.02, "comp > 0: autograd is the reference of the compensation VJP"
    # the visibility patterns
    mk = sc.masks
    assert not mk["none"].any() and mk["all"].all() and (0.15 < mk["mixed"].mean() < 0.45 or sc.N * sc.C < 50)
    for key, m in mk.items():
        if key.startswith("one@"):
            k = int(key[4:])
            assert m.sum() == 1 and m[sc.C - 1, k]
    if sc.N >= 256:
        w = mk["wave3"]
        assert not w[:, :192].any() and w[:, 192:256].all() and not w[:, 256:].any(), "waves 0-2 invisible as a whole, wave 3 full"
        assert "one@63" in mk and "one@64" in mk and "one@255" in mk
    if sc.C > 1:
        assert (mk["one-camera"].any(axis=1).sum() == 1)


def _masks_for(name):
    sc = R.scene(name)
    keys = [k for k in ("all", "mixed", "wave3", "one-camera", "one@63") if k in sc.masks]
    return keys if sc.C * sc.N < 10000 else ["mixed", "one-camera"]


def oracle_backward(oracle, name, mask, aa, with_vcomp, with_voe):
    """The C oracle on one call: name -> array, v_opac_eff folded by the caller (test_oracle_vs_torch_ref.py::oracle_backward)."""
    sc, f, cot = R.scene(name), R.scene_forward(name), R.cotangents(name)
    radii = sc.masks[mask].astype(np.int32) * 7
    v_comp = None
    if aa and (with_vcomp or with_voe):
        v_comp = np.zeros((sc.C, sc.N), np.float32)
        if with_vcomp:
            v_comp = v_comp + cot["v_comp"]
        if with_voe:
            v_comp = v_comp + cot["v_opac_eff"] * sc.opac[None]
    vm_, vq, vs, vvm = oracle.project_bwd(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, R.W, R.H, R.EPS2D, radii, f["conics32"],
                                          f["comp32"] if aa else None, cot["v_means2d"], cot["v_depths"], cot["v_conics"], v_comp)
    got = dict(means=vm_, quats=vq, scales=vs, viewmat=vvm)
    if with_voe:
        got["opacities"] = (cot["v_opac_eff"] * (f["comp32"] if aa else np.float32(1)) * sc.masks[mask]).sum(0)
    return got


def test_oracle_backward_within_constants(oracle):
    """Measures project_refs.ORACLE_BWD and asserts that the oracle still lies within it: a HIP kernel is allowed
    device_bound(constant) = four times max(constant, 1)."""
    worst = {k: 0.0 for k in R.OUTPUTS}
    for name in R.SCENES:
        for mask in _masks_for(name):
            for aa, wc, wo in OPTIONS:
                ref = R.reference(name, mask, aa, wc, wo)
                got = oracle_backward(oracle, name, mask, aa, wc, wo)
                for k, v in got.items():
                    val, terms = ref[k]
                    assert (np.abs(val) <= terms * (1 + 1e-9)).all()
                    w = R.worst_ratio(v, val, terms)
                    if w > worst[k]:
                        worst[k] = w
                        print(f"{name} {mask} aa={aa} v_comp={wc} v_opac_eff={wo}: {k} {w:.2f}")
    print("measured: ORACLE_BWD = " + ", ".join(f'"{k}": {v:.2f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert np.isfinite(v) and v <= R.ORACLE_BWD[k], (k, v)


def test_oracle_rows_of_invisible_pairs_are_zero(oracle):
    got = oracle_backward(oracle, "c3-n257", "none", True, True, True)
    assert not any(v.any() for v in got.values())
    ref = R.reference("c3-n257", "none")
    assert not any(val.any() or terms.any() for val, terms in ref.values())


def forward_scene():
    """The Gaussians of c3-n257 and c1-n600 in front of the three cameras of c3-n257, the clamped ones pulled half way inside and every
    fifth one enlarged: pairs on the screen, pairs off each of its four edges and pairs that reach it only through their radius."""
    a, b = R.scene("c3-n257"), R.scene("c1-n600")
    means = np.concatenate([a.means, b.means])
    scales = np.concatenate([a.scales, b.scales]).copy()
    scales[::5] *= 4.0
    return means, np.concatenate([a.quats, b.quats]), scales, a.viewmats, a.Ks


@pytest.mark.parametrize("clip", [0.0, 6.0])
def test_oracle_forward(oracle, clip):
    """Radii and cull decisions of the oracle equal the float64 reference's on every pair that is not within FWD_MARGIN of a
    threshold (at most 1 % of the pairs: asserted, the reference alone decides which); float outputs within ORACLE_FWD."""
    means, quats, scales, vm, K = forward_scene()
    f = R.forward(means, quats, scales, vm, K, radius_clip=clip)
    radii, m2, z, con, comp = oracle.project_fwd(means, quats, scales, vm, K, R.W, R.H, eps2d=R.EPS2D, near=R.NEAR, far=R.FAR,
                                                 radius_clip=clip, calc_compensations=True)
    ok = ~f["critical"]
    assert (~ok).mean() <= R.MAX_EXCLUDED, f"{(~ok).sum()} of {ok.size} pairs within the margin"
    assert np.array_equal(radii[ok], f["radii"][ok])
    vis = f["radii"] > 0
    assert 0.2 < vis.mean() < 0.9 and (clip == 0 or ((f["radii"] == 0) & (R.forward(means, quats, scales, vm, K)["radii"] > 0)).sum() > 20)
    terms = R.forward_terms(means, vm, K, f)
    keep = ok & vis
    worst = {}
    for key, got in (("means2d", m2), ("depths", z), ("conics", con), ("comp", comp)):
        worst[key] = R.worst_ratio(got[keep], f[key][keep], terms[key][keep])
        dead = ok & ~vis
        assert not got[dead].view(np.int32).any(), key + ": culled rows are +0"
    print("measured: ORACLE_FWD = " + ", ".join(f'"{k}": {v:.2f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= R.ORACLE_FWD[k], (k, v)


def _oracle_on_rows(oracle, rows, ids, with_vcomp=True):
    """The C oracle on compact rows of the large scene, scattered to dense arrays (the oracle has no compact path and no addends)."""
    sc, f = R.scene(R.BIG), R.scene_forward(R.BIG)
    N = sc.N
    radii = np.zeros((1, N), np.int32)
    radii[0, ids] = 2
    dense = {k: R.scatter(N, ids, np.asarray(v).astype(np.float32)) for k, v in rows.items()}
    v_comp = dense["v_opac_eff"] * sc.opac[None] + (dense["v_comp"] if with_vcomp else 0)
    vm_, vq, vs, vvm = oracle.project_bwd(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, R.W, R.H, R.EPS2D, radii, f["conics32"], f["comp32"],
                                          dense["v_means2d"], dense["v_depths"], dense["v_conics"], v_comp.astype(np.float32))
    return dict(means=vm_, quats=vq, scales=vs, viewmat=vvm, opacities=(dense["v_opac_eff"] * f["comp32"] * (radii > 0)).sum(0))


def test_oracle_on_the_compact_inputs(oracle):
    """The rows tests/test_gpu_project_edges.py feeds the compact path and the wire rows -- the scene's cotangents with their zero and
    single-cotangent rows, converted raw-moment rows, the wire rows of every case -- lie within the same constants project_refs.ORACLE_BWD."""
    worst = {k: 0.0 for k in R.OUTPUTS}

    def measure(tag, got, ref):
        for k, v in got.items():
            w = R.worst_ratio(v, *ref[k])
            if w > worst[k]:
                worst[k] = w
                print(f"{tag}: {k} {w:.2f}")

    for n_vis in R.NVIS:
        ids, rows, zero, d, only = R.compact_case(n_vis)
        assert (np.diff(ids) > 0).all() and ids.size == n_vis and (n_vis < 20 or 0.25 < zero.mean() < 0.55)
        for k in ("v_means2d", "v_depths", "v_conics", "v_comp", "v_opac_eff", "x_quat", "x_mean"):
            assert not rows[k][zero].any()
        assert len(only) == (5 if n_vis >= 5 else 1) and not zero[list(only)].any()
        for row, keep in only.items():                                     # live through exactly one input
            assert [k for k in ("v_means2d", "v_conics", "v_depths", "v_comp", "v_opac_eff", "x_quat", "x_mean") if rows[k][row].any()] == [keep]
        measure(f"compact {n_vis}", _oracle_on_rows(oracle, rows, ids), R.compact_reference(rows, ids, d, xq=False, xm=False))
        G, v_comp = R.raw_case(n_vis)
        k8 = R.eighth_only_row(n_vis)
        assert (k8 is None) == (n_vis < 5) and not G[zero].any()
        assert k8 is None or (not G[k8, :7].any() and G[k8, 7] != 0 and not G[k8, 8:].any() and v_comp[k8] == 0)
        rws, mags, conv, _ = R.row_gradients(G, ids, True, depth_col=11, v_comp=v_comp)
        measure(f"raw {n_vis}", _oracle_on_rows(oracle, rws, ids), R.compact_reference(rws, ids, d, xq=False, xm=False, mags=mags))
    modes, raws, depth_inside, depth_behind = set(), set(), 0, 0
    for n_vis, D, depth, mode, raw in R.wire_cases():
        ids, _, zero, d, _ = R.compact_case(n_vis)
        G, _ = R.wire_rows(n_vis, D, depth, bool(raw))
        assert G.shape[1] % 4 == 0 and G.shape[1] >= 8 + D + depth + 4 and (n_vis == 1 or (G[1, -1] != 0 and not G[1, :-1].any()))
        modes.add(mode); raws.add((mode, raw))
        depth_inside += bool(depth and D < 4); depth_behind += bool(depth and D >= 4)
        rws, mags, _, _ = R.row_gradients(G, ids, bool(raw), depth_col=8 + D if depth else None)
        measure(f"wire {n_vis} D={D} depth={depth} raw={raw}", _oracle_on_rows(oracle, rws, ids, with_vcomp=False),
                R.compact_reference(rws, ids, d, vcomp=False, xq=False, xm=False, mags=mags))
    assert modes == {0, 1, 2} and raws == {(m, r) for m in (0, 1, 2) for r in (0, 1)} and depth_inside >= 2 and depth_behind >= 2
    print("measured on the compact inputs: " + ", ".join(f'"{k}": {v:.2f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert np.isfinite(v) and v <= R.ORACLE_BWD[k], (k, v)


def test_oracle_flat_gaussians(oracle):
    """comp == 0: the scene has such pairs, the reference is finite there, and the oracle lies within ORACLE_BWD_FLAT of it."""
    a, fwd, mask, cot, ref = R.flat_case(oracle.project_fwd)
    assert mask.sum() >= 10 and ((fwd[0] > 0) & (fwd[4] > 0)).sum() >= 10, "flat pairs with comp == 0 and with a rounding residue > 0"
    assert (np.count_nonzero(a[2], axis=1) == 1).all()
    got = R.oracle_flat(oracle)
    worst = {}
    for k, v in got.items():
        val, terms = ref[k]
        assert np.isfinite(val).all() and np.isfinite(terms).all() and np.isfinite(v).all(), k
        worst[k] = R.worst_ratio(v, val, terms)
    print("measured: ORACLE_BWD_FLAT = " + ", ".join(f'"{k}": {v:.2f}' for k, v in worst.items()))
    assert not got["opacities"].any() and not ref["opacities"][0].any()
    # the division decides: the compensation's part carries 0.5 / 1e-6 and its terms dominate every other component's
    assert ref["means"][1][mask[0]].min() > 1e3 * np.abs(cot["v_means2d"]).max()
    for k, v in worst.items():
        assert v <= R.ORACLE_BWD_FLAT[k], (k, v)
