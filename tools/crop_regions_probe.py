"""Cropped decode of a region list against calls it does not touch: Batch.decode (RGBA) and Batch.decode_cropped with one
centred 224 x 224 rectangle, on the same resident frames in the same run.

256 resident frames (a few distinct pictures, each in several slots) of 3840x2160 4:2:2 DRI = 4 -- the benchmark's frames,
from tools/' synthetic encoder.  In one process, uploaded once: a few slots of every region row checked against the slice
of the batch's own RGBA decode, then, after a warm-up and with the clock primed, the rows timed in turn by device events
recorded on the stream around each row's call:
  yardsticks  RGBA by Batch.decode; decode_cropped of the centred 224 x 224
  row 1       the same centred rectangle as 256 regions
  row 2       a different random 224 x 224 rectangle per image (seeded)
  row 3       four random regions per image (1024 slots)
Then a second set: 128 of those frames and 128 of 1920x1080 4:2:0 DRI = 4, as two uniform batches and as one mixed batch:
  row 4       one centred 224 x 224 region per image of the mixed batch (two launches), against the sum of decode_cropped on
              the two uniform batches
  rows 4a, 4b the mixed batch's two launches each alone: the 4:2:2 images' regions, the 4:2:0 images' regions
Per row: the median with min .. max and the ratio to the row's yardstick.  No threshold is set for rows 2 to 4; below the
table, whether row 1 lies within the yardstick's own min .. max.  Needs the card: there is no CPU path.  Writes a table
(default profiles/crop_regions_decode.txt) and prints it.

    python tools/crop_regions_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/crop_regions_decode.txt]
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
    ap.add_argument("--check", type=int, default=3, help="slots compared with the slice of the RGBA decode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_regions_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)

    import compeg_amd as ca
    from tools import synth

    n, distinct, k = args.batch, min(args.distinct, args.batch), 4 if args.small else 1
    side = 224 // k
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(0xC0FFEE)
    w4, h4, w2, h2 = 3840 // k, 2160 // k, 1920 // k, 1080 // k
    big = [ca.ImageData(synth.make_jpeg(w4, h4, seed=0xC0FFEE + i, quality=85, ri=4)) for i in range(distinct)]
    small = [ca.ImageData(synth.make_jpeg(w2, h2, seed=0xC0FFEE + i, quality=85, ri=4, sampling=(2, 2)), allow_sampling=True) for i in range(distinct)]
    centre = lambda w, h: ((w - side) // 2, (h - side) // 2, side, side)
    lines = [f"cropped decode of a region list against untouched calls on the same frames: {n} resident frames ({distinct} distinct); {gpu.name()}",
             f"rows in turn, median of {args.reps} (min .. max); ms: device events on the stream around the row's call; slots of {side}x{side} rgba",
             f"{'frames':<34} {'row':<58} {'kernel':<9} {'slots':>6} {'ms':>28} {'ratio':>7}  to"]
    notes = []

    def timed(kinds, run, wait):
        for kind in kinds:   # warm-up: code objects, the planner's choices, the record stage
            for _ in range(2):
                run(kind)
                wait()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < PRIME_SECONDS:
            for kind in kinds:
                run(kind)
            wait()
        ms = {kind: [] for kind in kinds}
        for _ in range(args.reps):
            for kind in kinds:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                run(kind)
                b.record(stream)
                b.synchronize()
                ms[kind].append(a.elapsed_time(b))
        return ms

    def emit(frames, row, kernel, slots, t, base, to):
        med = statistics.median(t)
        lines.append(f"{frames:<34} {row:<58} {kernel:<9} {slots:>6} {med:>9.3f} ({min(t):.3f} .. {max(t):.3f}) {med / base:>7.3f}  {to}")

    def same_as_rgba(batch, dst, regions, slots):
        """The first --check slots of `dst` against the slice of the batch's own RGBA decode (already made)."""
        ok = True
        slot_bytes = 4 * side * side
        for s in slots:
            image, (x, y, rw, rh) = regions[s][0], regions[s][1]
            got = dst[s * slot_bytes:(s + 1) * slot_bytes].cpu().numpy().reshape(side, side, 4)
            ok = ok and bool(np.array_equal(got, batch.read_output(image)[y:y + rh, x:x + rw]))
        return ok

    # ---- rows 1 to 3: one uniform batch ----
    batch = ca.Batch(gpu)
    batch.upload([big[i % distinct] for i in range(n)])
    rect = centre(w4, h4)
    random_rect = lambda w, h: (int(rng.integers(0, w - side + 1)), int(rng.integers(0, h - side + 1)), side, side)
    lists = {"same": [(i, rect) for i in range(n)],
             "random": [(i, random_rect(w4, h4)) for i in range(n)],
             "four": [(i, random_rect(w4, h4)) for i in range(n) for _ in range(4)]}
    dst_one = torch.zeros(4 * side * side * n, dtype=torch.uint8, device="cuda")
    dsts = {name: torch.zeros(4 * side * side * len(regions), dtype=torch.uint8, device="cuda") for name, regions in lists.items()}
    batch.decode(stream.cuda_stream)
    batch.wait()
    for name, regions in lists.items():
        batch.decode_cropped_regions(dsts[name], regions, (side, side), hip_stream=stream.cuda_stream)
        batch.wait()
        slots = list(range(min(args.check, len(regions)))) + [len(regions) - 1]
        notes.append(f"row '{name}': slots {slots} equal the slice of the RGBA decode: {'yes' if same_as_rgba(batch, dsts[name], regions, slots) else 'NO'}")

    def run(kind):
        if kind == "rgba":
            batch.decode(stream.cuda_stream)
        elif kind == "one":
            batch.decode_cropped(dst_one, rect, hip_stream=stream.cuda_stream)
        else:
            batch.decode_cropped_regions(dsts[kind], lists[kind], (side, side), hip_stream=stream.cuda_stream)

    ms = timed(["rgba", "one", "same", "random", "four"], run, batch.wait)
    frames = f"{n} x {w4}x{h4} 422"
    rgba, one = statistics.median(ms["rgba"]), statistics.median(ms["one"])
    emit(frames, "yardstick: RGBA (Batch.decode)", "-", n, ms["rgba"], rgba, "itself")
    emit(frames, f"yardstick: decode_cropped, centred {side}x{side}", "cropped", n, ms["one"], rgba, "RGBA")
    emit(frames, "1: the same centred rectangle as a region per image", "cropped", n, ms["same"], one, "decode_cropped")
    emit(frames, "2: a random rectangle per image", "cropped", n, ms["random"], one, "decode_cropped")
    emit(frames, "3: four random regions per image", "cropped", 4 * n, ms["four"], statistics.median(ms["random"]), "row 2")
    med = statistics.median(ms["same"])
    inside = min(ms["one"]) <= med <= max(ms["one"])
    notes.append(f"row 1's median {med:.3f} ms lies {'within' if inside else 'OUTSIDE'} the decode_cropped yardstick's min .. max "
                 f"({min(ms['one']):.3f} .. {max(ms['one']):.3f}); it is {med - one:+.3f} ms ({(med / one - 1) * 100:+.1f} %) from its median")
    del batch, dsts, dst_one

    # ---- row 4: two uniform batches and one mixed batch ----
    half = n // 2
    b422, b420, mixed = ca.Batch(gpu), ca.Batch(gpu), ca.Batch(gpu)
    b422.upload([big[i % distinct] for i in range(half)])
    b420.upload([small[i % distinct] for i in range(half)])
    mixed.upload([(big if i % 2 == 0 else small)[(i // 2) % distinct] for i in range(2 * half)])   # (interleaved: the grouping sorts them)
    regions = [(i, centre(w4, h4) if i % 2 == 0 else centre(w2, h2)) for i in range(2 * half)]
    d422 = torch.zeros(4 * side * side * half, dtype=torch.uint8, device="cuda")
    d420 = torch.zeros(4 * side * side * half, dtype=torch.uint8, device="cuda")
    dmix = torch.zeros(4 * side * side * 2 * half, dtype=torch.uint8, device="cuda")
    mixed.decode(stream.cuda_stream)
    mixed.wait()
    mixed.decode_cropped_regions(dmix, regions, (side, side), hip_stream=stream.cuda_stream)
    mixed.wait()
    slots = list(range(min(args.check + 1, len(regions)))) + [len(regions) - 1]
    notes.append(f"row 4: slots {slots} equal the slice of the mixed batch's RGBA decode: {'yes' if same_as_rgba(mixed, dmix, regions, slots) else 'NO'}")

    halves = {"mixed 422": regions[0::2], "mixed 420": regions[1::2]}   # (the mixed batch's two launches, each alone)

    def run4(kind):
        if kind == "422":
            b422.decode_cropped(d422, centre(w4, h4), hip_stream=stream.cuda_stream)
        elif kind == "420":
            b420.decode_cropped(d420, centre(w2, h2), hip_stream=stream.cuda_stream)
        elif kind == "mixed":
            mixed.decode_cropped_regions(dmix, regions, (side, side), hip_stream=stream.cuda_stream)
        else:
            mixed.decode_cropped_regions(dmix, halves[kind], (side, side), hip_stream=stream.cuda_stream)

    def wait4():
        b422.wait(), b420.wait(), mixed.wait()

    ms = timed(["422", "420", "mixed", "mixed 422", "mixed 420"], run4, wait4)
    total = statistics.median(ms["422"]) + statistics.median(ms["420"])
    emit(f"{half} x {w4}x{h4} 422", f"yardstick: decode_cropped, centred {side}x{side}", "cropped", half, ms["422"], total, "the two yardsticks' sum")
    emit(f"{half} x {w2}x{h2} 420", f"yardstick: decode_cropped, centred {side}x{side}", "cropped", half, ms["420"], total, "the two yardsticks' sum")
    emit(f"{half} + {half} in one batch", "4: one centred region per image, two launches", "cropped", 2 * half, ms["mixed"], total, "the two yardsticks' sum")
    emit(f"{half} + {half} in one batch", "4a: the 4:2:2 images' regions alone, one launch", "cropped", half, ms["mixed 422"], statistics.median(ms["422"]), "the 422 yardstick")
    emit(f"{half} + {half} in one batch", "4b: the 4:2:0 images' regions alone, one launch", "cropped", half, ms["mixed 420"], statistics.median(ms["420"]), "the 420 yardstick")
    notes.append(f"row 4: the two uniform calls' medians add up to {total:.3f} ms")
    notes.append("not measured: hardware counters, single frames, other restart intervals, the planar format, pitched slots")
    lines += notes
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
