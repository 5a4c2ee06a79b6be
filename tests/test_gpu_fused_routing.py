"""Gradient routing of the one-node rasterization() (mtgs_amd/wrapper.py::_FusedRasterization): every gradient its backward returns
reaches the input it belongs to, and only that one, whichever inputs require a gradient -- with the dense gradients written into the
region the compositing backward clears (wrapper._backward_plan: zeroed) and with the streaming expansion pass."""
import pytest
import torch

pytestmark = pytest.mark.gpu

INPUTS = ("means", "quats", "scales", "opacities", "colors", "viewmats", "backgrounds")
N, W, H = 4096, 100, 60      # 7 x 4 tiles, the right and the bottom ones partial


def _run(requires, zeroed):
    """One forward + backward with `requires` requiring a gradient -> ({input: .grad or None}, entry points called, radii)."""
    from mtgs_amd import rasterization, wrapper
    from mtgs_amd.synthetic import make_camera, make_scene
    dev = torch.device("cuda")
    vm, K = make_camera(W, H, yaw_deg=5.0)
    g = torch.Generator().manual_seed(7)
    P = dict(make_scene(N, seed=3, sh_degree=None), viewmats=vm, backgrounds=torch.rand(1, 3, generator=g))
    P = {k: v.to(dev).requires_grad_(k in requires) for k, v in P.items()}
    calls, real, was = [], wrapper.call, wrapper._zeroed_outputs
    wrapper._zeroed_outputs = zeroed
    try:
        wrapper.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        render, alpha, info = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["colors"], P["viewmats"], K.to(dev),
                                            W, H, packed=False, render_mode="RGB+ED", absgrad=True, backgrounds=P["backgrounds"])
        Gc, Ga = torch.randn(render.shape, generator=g).to(dev), torch.randn(alpha.shape, generator=g).to(dev)
        ((render * Gc).sum() + (alpha * Ga).sum()).backward()
    finally:
        wrapper.call, wrapper._zeroed_outputs = real, was
    return {k: (None if P[k].grad is None else P[k].grad.clone()) for k in INPUTS}, calls, info["radii"][0]


@pytest.mark.parametrize("zeroed", [True, False], ids=["zeroed", "streamed"])
def test_every_gradient_reaches_its_own_input(hip_lib, zeroed):
    want, calls, radii = _run(INPUTS, zeroed)
    assert ("mtgs_project_bwd_zeroed" in calls) == zeroed and ("mtgs_project_bwd" in calls) == (not zeroed), calls
    visible = radii > 0
    n_vis = int(visible.sum())
    assert 0 < n_vis < N
    # some visible Gaussians have no gradient (occluded, or no pixel centre reached): rows the backward must leave zero
    assert bool((want["means"][visible] == 0).all(dim=1).any()) and bool((want["means"][visible] != 0).any())
    for k in INPUTS:
        assert want[k] is not None and bool((want[k] != 0).any()), k
    assert bool((want["means"][~visible] == 0).all())
    for k in INPUTS:
        got, calls_k, _ = _run((k,), zeroed)
        assert ("mtgs_project_bwd_zeroed" in calls_k) == zeroed, (k, calls_k)
        assert [o for o in INPUTS if got[o] is not None] == [k], k
        assert got[k].shape == want[k].shape
        assert torch.equal(got[k] != 0, want[k] != 0), k
        torch.testing.assert_close(got[k], want[k], rtol=1e-3, atol=1e-5 * float(want[k].abs().max()), msg=lambda m: f"{k}: {m}")
