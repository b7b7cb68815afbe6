"""Levels decode (a file's quantised DCT coefficients as int16 blocks) against its yardstick: the RGBA decode of the same
resident frames, in the same run.

Three batches of 256 resident frames (a few distinct pictures, each in several slots): 3840x2160 4:2:2 DRI = 4 -- the
benchmark's frames, from tools/' synthetic encoder --, 1920x1080 4:2:0 DRI = 4 from the same encoder, and 1920x1080
grayscale written by PIL with restart_marker_blocks = 8.  In one process, each batch uploaded once: the levels of the
distinct slots checked against the oracle's entropy pass (positions 0..31 through the quantiser: tests/levels_stream.py),
then, after a warm-up and with the clock primed, the rows timed in turn -- RGBA by Batch.decode, levels in zig-zag order,
levels in natural order, RGBA, ... -- by device events recorded on the stream around each row's calls.  Per row: the bytes
written per frame, the median with min .. max, and the ratio to the RGBA row.  No threshold is set: the table says what
was measured.  Needs the card: there is no CPU path.  Writes a table (default profiles/levels_decode.txt) and prints it.

    python tools/levels_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/levels_decode.txt]
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
    ap.add_argument("--reps", type=int, default=20, help="timed runs of each row, in turn")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/16 of the frame sizes")
    ap.add_argument("--check", type=int, default=2, help="distinct slots compared with the host expectation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)

    import compeg_amd as ca
    import levels_stream as ls
    import reduced_stream as rs
    from tools import synth

    n, distinct, k = args.batch, min(args.distinct, args.batch), 4 if args.small else 1
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    stream = torch.cuda.Stream()
    sets = (("422", 3840 // k, 2160 // k, dict(), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4)),
            ("420", 1920 // k, 1080 // k, dict(allow_sampling=True), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4, sampling=(2, 2))),
            ("gray", 1920 // k, 1080 // k, dict(allow_grayscale=True), lambda w, h, i: gray_jpeg(w, h, i)))
    lines = [f"levels decode (quantised DCT coefficients, int16 blocks) against the RGBA decode of the same frames: {n} resident frames ({distinct} distinct) a batch; {gpu.name()}",
             f"rows in turn (RGBA, levels zigzag, levels natural, RGBA, ...), median of {args.reps} (min .. max); ms: device events on the",
             "stream around the row's calls; out B/frame: bytes the row writes per frame; vs RGBA: the row's median over the RGBA row's",
             f"{'frames':<22} {'row':<28} {'kernel':<13} {'out B/frame':>12} {'ms':>28} {'vs RGBA':>8}"]
    notes = []
    for layout, w, h, kw, make in sets:
        jpegs = [make(w, h, i) for i in range(distinct)]
        images = [ca.ImageData(j, **kw) for j in jpegs]
        hs, vs = images[0].sampling()
        comps = images[0].components()
        batch = ca.Batch(gpu)
        batch.upload([images[i % distinct] for i in range(n)])
        total = ca.levels_shape(w, h, (hs, vs), comps)[1]
        dst = torch.zeros(total * n, dtype=torch.uint8, device="cuda")
        # the levels against the oracle's entropy pass, on a few of the distinct slots
        same = True
        for order in ls.ORDERS:
            batch.decode_levels(dst, order, hip_stream=stream.cuda_stream)
            batch.wait()
            for i in range(min(args.check, distinct)):
                coef, (_, _, _, _, _, dpm, mcus_w, mcus_h), _ = rs.file_coefficients(ca, jpegs[i], **kw)
                want = ls.rasters(coef, mcus_w, mcus_h, comps, hs, vs)
                got = ls.views(dst[i * total:(i + 1) * total].cpu().numpy(), w, h, comps, hs, vs)
                for c in range(comps):
                    grid, mask = want[c]
                    deq = ls.dequantised_low(got[c], batch.quant_table(i, c), order)
                    same = same and bool(mask.all()) and bool(np.array_equal(deq, grid[..., :32]))
        notes.append(f"{layout}: levels x quantiser equal the oracle's coefficients at positions 0..31 on {min(args.check, distinct)} slots, both orders: {'yes' if same else 'NO'}")

        def run(kind):
            if kind == "full":
                batch.decode(stream.cuda_stream)
            else:
                batch.decode_levels(dst, kind, hip_stream=stream.cuda_stream)

        kinds = ["full"] + list(ls.ORDERS)
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
        for _ in range(args.reps):
            for kind in kinds:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                run(kind)
                b.record(stream)
                b.synchronize()
                ms[kind].append(a.elapsed_time(b))
        base = statistics.median(ms["full"])
        for kind in kinds:
            t = ms[kind]
            med = statistics.median(t)
            out_bytes = 4 * w * h if kind == "full" else total
            row = "RGBA (Batch.decode)" if kind == "full" else f"levels {kind}"
            lines.append(f"{f'{w}x{h} {layout}':<22} {row:<28} {names[kind]:<13} {out_bytes:>12} "
                         f"{med:>9.3f} ({min(t):.3f} .. {max(t):.3f}) {med / base:>8.3f}")
        del batch, dst
    lines += notes
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
