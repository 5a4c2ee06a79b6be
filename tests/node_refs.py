"""Plain references of the per-Gaussian operators around the scene graph (csrc/fourier.hip, deform.hip, stats.hip, oob.hip;
refinement has its own in oracle/refine_oracle.py), one function per operator: NumPy / torch on the CPU, float64 unless the
kernel's header comment fixes a float32 step, written out from the formula that comment states.  TEST INFRASTRUCTURE ONLY;
nothing under mtgs_amd/ imports this.

Conventions
  * inputs are the float32 (and int32) CPU arrays the device call receives;
  * where the kernel forms an ARGUMENT in float32 (x = means / height * 2 of the embedding) the reference forms the same
    float32 number and only then goes to float64, so that sin(x 2^15) is asked of the same x;
  * the statistics references update their arrays in place, as the operator does, in the dtype of the arrays they are given.
"""
import numpy as np
import torch

from tests.image_refs import oob_ref  # noqa: F401  (the out-of-box reference is the one of the image-space tests)

U32 = 2.0 ** -24          # unit roundoff of float32


# ---- Fourier colour -------------------------------------------------------------------------------------------------------------
def fourier_ref(features_dc, w, v_dc):
    """fourier.hip: dc[n,:] = sum_f features_dc[n,f,:] w[f];  v_features_dc[n,f,:] = w[f] v_dc[n,:];
    v_w[f] = sum_n <features_dc[n,f,:], v_dc[n,:]>.  features_dc [N,F,3], w [F], v_dc [N,3].
    Returns (dc, v_features_dc, v_w, abs_terms_w) in float64, abs_terms_w[f] = sum_n |<features_dc[n,f,:], v_dc[n,:]>|:
    the scale of the rounding error of a float32 evaluation of v_w[f]."""
    f = np.asarray(features_dc, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    g = np.asarray(v_dc, dtype=np.float64)
    dc = np.einsum("nfc,f->nc", f, w)
    v_f = w[None, :, None] * g[:, None, :]
    terms = np.einsum("nfc,nc->nf", f, g)
    return dc, v_f, terms.sum(0), np.abs(terms).sum(0)


# ---- deformation embedding ------------------------------------------------------------------------------------------------------
def deform_embed_width(x_freqs, t_freqs, E):
    return 3 + 6 * x_freqs + 1 + 2 * t_freqs + E


def deform_embed_args(means, height, t, x_freqs, t_freqs):
    """The float32 arguments of every sin / cos of the row matrix: (x 2^i [N, x_freqs, 3], t 2^i [t_freqs]) with
    x = means / height * 2 formed in float32 as the kernel forms it (a power of two scales a float32 exactly)."""
    x = np.asarray(means, dtype=np.float32).reshape(-1, 3) / np.float32(height) * np.float32(2)
    fx = np.float32(2) ** np.arange(x_freqs, dtype=np.float32)
    ft = np.float32(2) ** np.arange(t_freqs, dtype=np.float32)
    return x, x[:, None, :] * fx[None, :, None], np.float32(t) * ft


def deform_embed_ref(means, height, t, cond, x_freqs, t_freqs):
    """deform.hip: row n = [x | sin(x f_i), cos(x f_i) for i < x_freqs | t | sin(t f_i), cos(t f_i) for i < t_freqs | cond],
    f_i = 2^i, x = means[n] / height * 2 in float32, sin / cos in float64.  Returns [N, 3 + 6 x_freqs + 1 + 2 t_freqs + E]."""
    x, ax, at = deform_embed_args(means, height, t, x_freqs, t_freqs)
    N = x.shape[0]
    cols = [x.astype(np.float64)]
    for i in range(x_freqs):
        cols += [np.sin(ax[:, i].astype(np.float64)), np.cos(ax[:, i].astype(np.float64))]
    tail = [np.float64(np.float32(t))]
    for i in range(t_freqs):
        tail += [np.sin(np.float64(at[i])), np.cos(np.float64(at[i]))]
    tail = np.concatenate([np.asarray(tail, dtype=np.float64), np.asarray(cond, dtype=np.float64).reshape(-1)])
    return np.concatenate(cols + [np.repeat(tail[None], N, 0)], axis=1)


# ---- densification statistics ---------------------------------------------------------------------------------------------------
def stats_ref(stats, radii, xys_grad, submodel_mask, W, H):
    """update_submodel_statistics + after_train for one node, the masked-tensor formulation stats.hip cites, in place on
    stats = [xys_grad_norm, vis_counts, max_2Dsize] (CPU tensors): radii [1,N], xys_grad [1,N,2] (absgrad or grad),
    submodel_mask [N] bool."""
    xys_grad_norm, vis_counts, max_2Dsize = stats
    grads = xys_grad[0, submodel_mask].detach()
    image_size = grads.new_tensor([W, H]).unsqueeze(0)
    grads = (grads * image_size * 0.5).norm(dim=-1)
    node_radii = radii[0, submodel_mask]
    visible_mask = (node_radii > 0).flatten()
    vis_counts[visible_mask] += +1
    xys_grad_norm[visible_mask] += grads[visible_mask]
    newradii = node_radii.detach()[visible_mask]
    max_2Dsize[visible_mask] = torch.maximum(max_2Dsize[visible_mask], newradii)


def stats_ref_rows(stats, starts, radii, rows, vis_ids, W, H, col=2, count=None):
    """The same update from compact gradient rows (mtgs_densify_stats_rows): row r < count belongs to the Gaussian with flat
    index vis_ids[r], its 2-D gradient sits in columns col, col + 1 of rows[r] (0: the plain gradient, 2: the absgrad), and
    it is visible by construction.  stats[i] = [xys_grad_norm, vis_counts, max_2Dsize] of the node that owns the flat
    indices [starts[i], starts[i] + n_i); an index that no listed node owns is skipped.  Written as the dense update of
    the scattered rows: a dense gradient that is zero, and a radius that is zero, wherever no row points."""
    radii = radii.reshape(-1)
    N = radii.numel()
    count = vis_ids.numel() if count is None else int(count)
    ids = vis_ids[:count].long()
    assert ids.unique().numel() == count, "one row per visible Gaussian"
    dtype = stats[0][0].dtype if stats else torch.float64
    dense = torch.zeros(1, N, 2, dtype=dtype)
    dense[0, ids] = rows[:count, col:col + 2].to(dtype)
    listed = torch.zeros(1, N, dtype=dtype)
    listed[0, ids] = radii[ids].to(dtype)
    assert bool((listed[0, ids] > 0).all()), "a listed Gaussian is a visible one"
    for s, st in zip(stats, starts):
        mask = torch.zeros(N, dtype=torch.bool)
        mask[st:st + s[0].numel()] = True
        stats_ref(s, listed, dense, mask, W, H)
