"""Planes decode against its own yardstick: the RGBA decode of the same resident frames, in the same run.

Three batches of 256 resident frames (a few distinct pictures, each in several slots): 3840x2160 4:2:2 DRI = 4 -- the
benchmark's frames, from tools/' synthetic encoder --, 1920x1080 4:2:0 DRI = 4 from the same encoder, and 1920x1080
grayscale written by PIL with restart_marker_blocks = 8.  In one process, each batch uploaded once: the planes of a few
slots checked against the RGBA decode through the host colour step, then, after a warm-up and with the clock primed, the
decodes timed in turn -- RGBA by Batch.decode, planes in each format the sampling takes, RGBA, ... -- by device events
recorded on the decode's stream around each call (the same way for both kinds; for RGBA the batch's own
compeg_batch_timing is printed beside it).  Per row: the bytes written per frame, the algorithmic bytes of DESIGN.md 5.1
with the output term replaced, and their share of the 8 TB/s roofline at the measured time.  Needs the card: there is no
CPU path.  Writes a table (default profiles/planes_decode.txt) and prints it.

    python tools/planes_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/planes_decode.txt]
"""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PRIME_SECONDS = 0.08
HBM_BYTES_PER_S = 8.0e12
FORMATS = {"422": (("planar", "coded"), ("semiplanar", "coded"), ("yuyv", "coded"), ("uyvy", "coded"), ("planar", "420"), ("semiplanar", "420")),
           "420": (("planar", "coded"), ("semiplanar", "coded")), "gray": (("planar", "coded"),)}


def gray_jpeg(w, h, seed):
    from PIL import Image
    from gray_probe import picture
    out = io.BytesIO()
    Image.fromarray(picture(w, h, seed), "L").save(out, "JPEG", quality=85, restart_marker_blocks=8)
    return out.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20, help="timed decodes of each kind, in turn")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/16 of the frame sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)

    import compeg_amd as ca
    import planes_stream as ps
    from tools import synth

    n, distinct, k = args.batch, min(args.distinct, args.batch), 4 if args.small else 1
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    stream = torch.cuda.Stream()
    sets = (("422", 3840 // k, 2160 // k, dict(), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4)),
            ("420", 1920 // k, 1080 // k, dict(allow_sampling=True), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4, sampling=(2, 2))),
            ("gray", 1920 // k, 1080 // k, dict(allow_grayscale=True), lambda w, h, i: gray_jpeg(w, h, i)))
    lines = [f"planes decode against the RGBA decode of the same frames: {n} resident frames ({distinct} distinct) a batch; {gpu.name()}",
             f"decodes in turn (RGBA, every planes format, RGBA, ...), median of {args.reps} (min .. max); ms: device events on the decode's stream around",
             "the call; (timing): compeg_batch_timing's figure for the same RGBA decodes; out B/frame: bytes the decode writes per frame; alg MB: inputs +",
             "outputs of the batch (DESIGN.md 5.1, the output term replaced); roofline: alg bytes / 8 TB/s / ms",
             f"{'frames':<22} {'output':<18} {'kernel':<13} {'out B/frame':>12} {'alg MB':>9} {'ms':>28} {'vs RGBA':>8} {'roofline':>9}"]
    notes = []
    for layout, w, h, kw, make in sets:
        jpegs = [make(w, h, i) for i in range(distinct)]
        images = [ca.ImageData(j, **kw) for j in jpegs]
        comps, (hs, vs) = images[0].components(), images[0].sampling()
        batch = ca.Batch(gpu)
        batch.upload([images[i % distinct] for i in range(n)])
        inputs = batch.algorithmic_bytes() - 4 * w * h * n
        dests = {}
        for format, chroma in FORMATS[layout]:
            total = ca.planes_shape(w, h, (hs, vs), comps, format, chroma)[1]
            dests[(format, chroma)] = (torch.zeros(total * n, dtype=torch.uint8, device="cuda"), total)
        # the same picture both ways, on the distinct slots
        batch.decode(stream.cuda_stream)
        batch.wait()
        rgba = [batch.read_output(i) for i in range(distinct)]
        dst, total = dests[("planar", "coded")]
        batch.decode_planes(dst, "planar", "coded", hip_stream=stream.cuda_stream)
        batch.wait()
        same = True
        for i in range(distinct):
            got = dst[i * total:(i + 1) * total].cpu().numpy()
            y, cb, cr = (ps.views(got, w, h, comps, hs, vs) + [None, None])[:3]
            same = same and bool(np.array_equal(ps.colour(y, cb, cr, hs, vs, w, h, rgba[i][..., 3] == 255), rgba[i]))
        notes.append(f"{layout}: planes through the host colour step equal the RGBA decode on {distinct} slots: {'yes' if same else 'NO'}")

        def run(kind):
            if kind == "rgba":
                batch.decode(stream.cuda_stream)
            else:
                batch.decode_planes(dests[kind][0], kind[0], kind[1], hip_stream=stream.cuda_stream)

        kinds = ["rgba"] + list(FORMATS[layout])
        names = {}
        for kind in kinds:   # warm-up: code objects, the planner's choices
            for _ in range(2):
                run(kind)
                batch.wait()
            names[kind] = batch.last_kernel()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < PRIME_SECONDS:
            for kind in kinds:
                run(kind)
            batch.wait()
        ms = {kind: [] for kind in kinds}
        timing_ms = []
        for _ in range(args.reps):
            for kind in kinds:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if kind == "rgba":
                    batch.timing(reset=True)
                a.record(stream)
                run(kind)
                b.record(stream)
                b.synchronize()
                ms[kind].append(a.elapsed_time(b))
                if kind == "rgba":
                    timing_ms.append(batch.timing(reset=True)[1])
        base = statistics.median(ms["rgba"])
        for kind in kinds:
            t = ms[kind]
            med = statistics.median(t)
            out_bytes = 4 * w * h if kind == "rgba" else dests[kind][1]
            alg = inputs + out_bytes * n
            label = "RGBA" if kind == "rgba" else f"{kind[0]}" + ("+420" if kind[1] == "420" else "")
            lines.append(f"{f'{w}x{h} {layout}':<22} {label:<18} {names[kind]:<13} {out_bytes:>12} {alg / 1e6:>9.1f} "
                         f"{med:>9.3f} ({min(t):.3f} .. {max(t):.3f}) {med / base:>8.3f} {alg / HBM_BYTES_PER_S / (med * 1e-3):>8.1%}")
        lines.append(f"{'':<22} {'RGBA (timing)':<18} {'':<13} {'':>12} {'':>9} {statistics.median(timing_ms):>9.3f} ({min(timing_ms):.3f} .. {max(timing_ms):.3f})")
        del batch, dests
    lines += notes
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
