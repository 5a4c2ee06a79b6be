"""One SHA-256 per (step, node) of what refine_gaussians (followed, at the reset step, by reset_opacities) returns for the nodes
of tests/refine_scene_refs.identity_scene(): every parameter, both moments of each, the extras, src_index, kind, the counts and
the mask its hook received.  Public API and the shared fixtures only, so the script runs unchanged on any commit: two digests
taken on the same machine from two commits are byte-identical exactly when refine_gaussians computes the same bits.

    python scripts/refine_digest.py OUT.txt

The digest is not a fixture: its bits depend on the device math library."""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mtgs_amd.densify import refine_gaussians, reset_opacities  # noqa: E402
from tests import refine_scene_refs as R  # noqa: E402

COUNTS = ("n_before", "n_after", "n_old_kept", "n_children", "n_dups", "n_split")


def main(out):
    up = lambda a: torch.from_numpy(a).cuda()
    lines = []
    for step in R.IDENTITY_STEPS + (R.RESET_STEP,):
        for i, (p, stats, moments, extras, cfg, seed) in enumerate(R.identity_scene()):
            masks = []
            new, new_m, info = refine_gaussians({k: up(v) for k, v in p.items()}, tuple(up(s) for s in stats), cfg, step, seed,
                                                moments={k: (up(a), up(b)) for k, (a, b) in moments.items()},
                                                extras={k: up(v) for k, v in extras.items()}, before_rows=masks.append)
            if step == R.RESET_STEP:
                reset_opacities(new["opacities"], cfg, new_m["opacities"])
            h = hashlib.sha256(repr([int(info[k]) for k in COUNTS]).encode())
            tensors = [(k, new[k]) for k in sorted(new)] + [(f"{k}.m{j}", new_m[k][j]) for k in sorted(new_m) for j in (0, 1)]
            tensors += [(f"x.{k}", info["extras"][k]) for k in sorted(info["extras"])] + [("src_index", info["src_index"]), ("kind", info["kind"])]
            tensors += [("mask", m) for m in masks]
            for name, t in tensors:
                h.update(f"{name}{tuple(t.shape)}{t.dtype}".encode())
                h.update(t.contiguous().cpu().numpy().tobytes())
            lines.append(f"{step} {i} {h.hexdigest()}")
    Path(out).write_text("\n".join(lines) + "\n")
    print(f"{out}: {len(lines)} lines")


if __name__ == "__main__":
    main(sys.argv[1])
