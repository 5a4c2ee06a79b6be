#!/usr/bin/env python
"""Times the decode of a baseline JPEG frame: mtgs_amd.jpegdec on the device against what it replaces, Pillow's decode on the host
followed by the `.cuda()` of its pixels (the reference's Image.open + np.array, mtgs/dataset/custom_dataset.py:78-97).

    1920 x 1080, 910 x 512, 228 x 128; Pillow's files at quality 75 and 95, 4:2:0 and 4:4:4, of the image kinds of the encoder's
    tests (noise, ramp, checker, blocks, constant) and of one rendered-looking frame (scripts/jpeg_bench.py's)

The device path is timed with HIP events around the whole call, from host bytes (parse and upload included) and from a DeviceJpeg
with `out` and `workspace` given (the compressed cache); the host path with the host clock around a decode that ends with the pixels
on the device: the median and the spread of `--reps` after `--warmup`.  The pixels of the two paths are compared before timing.
The four candidate values of subsequence_bits are timed at 1920 x 1080, quality 75, 4:2:0 (the frame), and the per-kernel split is
torch.profiler's device time per kernel name there, with every synchronisation launch of one decode on its own: the ones that
work and the ones that find the flag clear and return.  Writes profiles/jpegdec.txt.

    python scripts/jpegdec_bench.py [--reps 20] [--warmup 5] [--out profiles/jpegdec.txt]
"""
import argparse
import io
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from jpeg_bench import device_events, fmt, frame, host_clock, kernel_split  # noqa: E402
from mtgs_amd import jpegdec as J  # noqa: E402

SIZES = [(1080, 1920), (512, 910), (128, 228)]
KINDS = ("frame", "noise", "ramp", "checker", "blocks", "constant")
CANDIDATES = (512, 1024, 2048, 4096)


def image(kind, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "frame":
        return frame(h, w, h + 75)
    if kind == "noise":
        return np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "ramp":
        return np.stack([(255 * xx) // (w - 1), (255 * yy) // (h - 1), (255 * (xx + yy)) // (h + w - 2)], -1).astype(np.uint8)
    if kind == "checker":
        return np.repeat((((yy + xx) & 1) * 255)[..., None], 3, -1).astype(np.uint8)
    if kind == "blocks":
        return np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255)[..., None], 3, -1).astype(np.uint8)
    return np.full((h, w, 3), (200, 30, 90), dtype=np.uint8)


def sync_launches(fn):
    """device us of every jpegdec_sync_kernel launch of ONE decode, in launch order; None if torch.profiler reports nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        events = [ev for ev in prof.events() if "jpegdec_sync_kernel" in ev.name and str(ev.device_type).endswith("CUDA")]
        events.sort(key=lambda ev: ev.time_range.start)
        return [float(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0)) for ev in events] or None
    except Exception as exc:                    # a report, not a result
        print(f"torch.profiler: {exc!r}", file=sys.stderr)
        return None


def report_sync_launches(emit, jpeg, out, ws, every):
    each = sync_launches(lambda: J.decode_jpeg(jpeg, out=out, workspace=ws))
    if each:
        idle = [x for x in each if x < 0.1 * max(each)]
        if every:
            emit(f"    the {len(each)} synchronisation launches of one decode, us each: " + " ".join(f"{x:.1f}" for x in each))
        emit(f"    of {len(each)} synchronisation launches {len(each) - len(idle)} did work ({sum(each) - sum(idle):.1f} us); the {len(idle)} that found "
             f"the flag clear cost {sum(idle):.1f} us together" + (f", {sum(idle) / len(idle):.1f} us each" if idle else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jpegdec.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jpegdec_bench.py measures on the device: there is no CPU timing"
    import PIL
    from PIL import Image, features
    lines = [f"mtgs_amd.jpegdec against Pillow's decode + .cuda() (Pillow {PIL.__version__}, libjpeg-turbo {features.version('jpg')}), "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"device: HIP events around the whole call; host: the host clock around a decode that ends on the device; median (min .. max) of "
             f"{a.reps} after {a.warmup} warm-ups; subsequence_bits {J.SUBSEQUENCE_BITS} unless said", ""]

    def save(pixels, **kw):
        with tempfile.TemporaryDirectory() as tmp:
            Image.fromarray(pixels).save(Path(tmp) / "x.jpg", "JPEG", **kw)
            return (Path(tmp) / "x.jpg").read_bytes()

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    for h, w in SIZES:
        for kind in KINDS:
            pixels = image(kind, h, w)
            for q in (75, 95):
                for s, sub in (("4:2:0", 2), ("4:4:4", 0)):
                    data = save(pixels, quality=q, subsampling=sub)
                    host = lambda: torch.from_numpy(np.array(Image.open(io.BytesIO(data)))).cuda()
                    jpeg = J.upload_jpeg(data)
                    out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
                    ws = torch.empty(J.sizes(jpeg.info), dtype=torch.uint8, device="cuda")
                    _, status = J.decode_jpeg(jpeg, out=out, workspace=ws, return_status=True)
                    status = status.cpu().tolist()
                    same = torch.equal(out, host()) and torch.equal(J.decode_jpeg(data), out)
                    t_host = host_clock(lambda: (host(), torch.cuda.synchronize()), a.reps, a.warmup)
                    t_bytes = device_events(lambda: J.decode_jpeg(data, out=out, workspace=ws), a.reps, a.warmup)
                    t_cache = device_events(lambda: J.decode_jpeg(jpeg, out=out, workspace=ws), a.reps, a.warmup)
                    emit(f"{w} x {h} {kind:8s} q{q} {s}: file {len(data):8d} bytes ({pixels.nbytes / len(data):6.1f}x fewer than the pixels), "
                         f"identical {same}, status {status} (about {jpeg.info.scan_length * 8 // J.SUBSEQUENCE_BITS + 1} subsequences, from the raw scan's length)")
                    emit(f"    host: Pillow + .cuda()             {fmt(t_host)}")
                    emit(f"    device, from host bytes            {fmt(t_bytes)}    host / device {statistics.median(t_host) / statistics.median(t_bytes):5.2f}x")
                    emit(f"    device, from a DeviceJpeg          {fmt(t_cache)}    host / device {statistics.median(t_host) / statistics.median(t_cache):5.2f}x")
                    if (h, w, kind, q, s) == (1080, 1920, "noise", 95, "4:4:4"):          # the longest stream: the most launches
                        report_sync_launches(emit, jpeg, out, ws, every=False)
                    if (h, w, kind, q, s) == (1080, 1920, "frame", 75, "4:2:0"):
                        emit("    subsequence_bits at this case (the default is the fastest of these):")
                        for bits in CANDIDATES:
                            wsb = torch.empty(J.sizes(jpeg.info, bits), dtype=torch.uint8, device="cuda")
                            _, st = J.decode_jpeg(jpeg, out=out, workspace=wsb, subsequence_bits=bits, return_status=True)
                            t = device_events(lambda: J.decode_jpeg(jpeg, out=out, workspace=wsb, subsequence_bits=bits), a.reps, a.warmup)
                            emit(f"      {bits:5d} bits  {fmt(t)}   synchronisation launches that changed an entry: {st.cpu().tolist()[3]}")
                        report_sync_launches(emit, jpeg, out, ws, every=True)
                        split = kernel_split(lambda: J.decode_jpeg(jpeg, out=out, workspace=ws), a.reps)
                        if split:
                            emit("    per kernel (torch.profiler, device us per decode, launches per decode):")
                            for name, us, count in split:
                                emit(f"      {us:8.1f} us  x{count:.0f}  {name[:130]}")
        emit("")
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()
