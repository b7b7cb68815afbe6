"""Cropped decode against its own yardsticks: the RGBA decode of the same resident frames, and that decode followed by the
pack that crops it (pack_tensor_regions of the same rectangle at scale 1), in the same run.

Two batches of 256 resident frames (a few distinct pictures, each in several slots): 3840x2160 4:2:2 DRI = 4 -- the
benchmark's frames, from tools/' synthetic encoder -- and 1920x1080 4:2:0 DRI = 4 from the same encoder.  In one process,
each batch uploaded once: two slots of every cropped row checked against the slice of the batch's own RGBA decode, then,
after a warm-up and with the clock primed, the rows timed in turn -- RGBA by Batch.decode, cropped full frame, cropped
centred half x half, cropped centred 224 x 224, cropped 224 x 224 in the last MCU rows, the chain Batch.decode +
pack_tensor_regions of the centred 224 x 224, RGBA, ... -- by device events recorded on the stream around each row's calls.
Per row: the bytes written per frame, the median with min .. max, and the ratio to the RGBA row.  Below the table: whether
each 224 x 224 row is faster than the RGBA row by more than the two rows' min .. max spreads added together.  No other
threshold is set: the table says what was measured.  Needs the card: there is no CPU path.  Writes a table (default
profiles/crop_decode.txt) and prints it.

    python tools/crop_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/crop_decode.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PRIME_SECONDS = 0.08


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20, help="timed runs of each row, in turn")
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/4 of the frame sizes")
    ap.add_argument("--check", type=int, default=2, help="slots compared with the slice of the RGBA decode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)

    import compeg_amd as ca
    from tools import synth

    n, distinct, k = args.batch, min(args.distinct, args.batch), 4 if args.small else 1
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    stream = torch.cuda.Stream()
    sets = (("422", 3840 // k, 2160 // k, dict(), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4)),
            ("420", 1920 // k, 1080 // k, dict(allow_sampling=True), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4, sampling=(2, 2))))
    lines = [f"cropped decode against the RGBA decode of the same frames: {n} resident frames ({distinct} distinct) a batch; {gpu.name()}",
             f"rows in turn (RGBA, cropped full, half, 224 centre, 224 last rows, RGBA + pack_tensor_regions, RGBA, ...), median of {args.reps} (min .. max); ms:",
             "device events on the stream around the row's calls; out B/frame: bytes the row writes per frame; vs RGBA: the row's median over the RGBA row's",
             f"{'frames':<18} {'row':<48} {'kernel':<13} {'out B/frame':>12} {'ms':>28} {'vs RGBA':>8}"]
    notes = []
    for layout, w, h, kw, make in sets:
        jpegs = [make(w, h, i) for i in range(distinct)]
        images = [ca.ImageData(j, **kw) for j in jpegs]
        batch = ca.Batch(gpu)
        batch.upload([images[i % distinct] for i in range(n)])
        side = 224 // k
        rects = {"full": (0, 0, w, h),
                 "half": (w // 4, h // 4, w // 2, h // 2),
                 "224 centre": ((w - side) // 2, (h - side) // 2, side, side),
                 "224 last rows": ((w - side) // 2 + 3, h - side, side, side)}
        dests = {}
        for name, rect in rects.items():
            total = ca.crop_shape(w, h, rect)[1]
            dests[name] = (torch.zeros(total * n, dtype=torch.uint8, device="cuda"), total)
        crop = rects["224 centre"]
        packed = torch.zeros((n, 3, side, side), dtype=torch.uint8, device="cuda")
        regions = [(i, crop, None) for i in range(n)]   # (the crop into the whole slot: scale 1)
        # the cropped images against the slice of the batch's own RGBA decode, on a few slots
        batch.decode(stream.cuda_stream)
        batch.wait()
        full = [batch.read_output(i) for i in range(min(args.check, n))]
        same = True
        for name, (x, y, rw, rh) in rects.items():
            dst, total = dests[name]
            batch.decode_cropped(dst, rects[name], hip_stream=stream.cuda_stream)
            batch.wait()
            for i, rgba in enumerate(full):
                got = dst[i * total:(i + 1) * total].cpu().numpy().reshape(rh, rw, 4)
                same = same and bool(np.array_equal(got, rgba[y:y + rh, x:x + rw]))
        notes.append(f"{layout}: cropped images equal the slice of the RGBA decode on {len(full)} slots, all four rectangles: {'yes' if same else 'NO'}")

        def run(kind):
            if kind == "rgba":
                batch.decode(stream.cuda_stream)
            elif kind == "chain":
                batch.decode(stream.cuda_stream)
                batch.pack_tensor_regions(packed, (side, side), regions, dtype="u8", hip_stream=stream.cuda_stream)
            else:
                batch.decode_cropped(dests[kind][0], rects[kind], hip_stream=stream.cuda_stream)

        kinds = ["rgba"] + list(rects) + ["chain"]
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
        base = statistics.median(ms["rgba"])
        label = {"rgba": "RGBA (Batch.decode)", "chain": f"RGBA + pack_tensor_regions({side}x{side}, u8)"}
        for kind in kinds:
            t = ms[kind]
            med = statistics.median(t)
            out_bytes = {"rgba": 4 * w * h, "chain": 4 * w * h + 3 * side * side}.get(kind) or dests[kind][1]
            row = label.get(kind) or f"cropped {kind} {rects[kind][2]}x{rects[kind][3]} at ({rects[kind][0]}, {rects[kind][1]})"
            lines.append(f"{f'{w}x{h} {layout}':<18} {row:<48} {names[kind]:<13} {out_bytes:>12} "
                         f"{med:>9.3f} ({min(t):.3f} .. {max(t):.3f}) {med / base:>8.3f}")
        for kind in ("224 centre", "224 last rows"):
            gap = base - statistics.median(ms[kind])
            spreads = (max(ms["rgba"]) - min(ms["rgba"])) + (max(ms[kind]) - min(ms[kind]))
            notes.append(f"{layout}: cropped {kind} is {gap:.3f} ms below the RGBA row; the two rows' spreads together are {spreads:.3f} ms: "
                         f"the condition {'holds' if gap > spreads else 'DOES NOT HOLD'}")
        del batch, dests, packed
    lines += notes
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
