"""Scaled (1/2- and 1/4-scale) decode against its own yardsticks: the RGBA decode of the same resident frames (code the
scaled decode does not touch), the reduced (1/8) decode, and the chains the scaled decode replaces -- the RGBA decode
followed by the pack that shrinks it (pack_tensor(downscale=2 | 4, u8)) -- in the same run.

Two batches of 256 resident frames (a few distinct pictures, each in several slots): 3840x2160 4:2:2 DRI = 4 -- the
benchmark's frames, from tools/' synthetic encoder -- and 1920x1080 4:2:0 DRI = 4 from the same encoder.  In one process,
each batch uploaded once: the scaled image of a few distinct slots checked against tests/scaled_stream.py, then, after a
warm-up and with the clock primed, the rows timed in turn -- RGBA by Batch.decode, reduced, scaled 1/2 and 1/4 in both
formats, the two chains, RGBA, ... -- by device events recorded on the stream around each row's calls.  Per row: the bytes
written per frame, the median with min .. max, and the ratio to the RGBA row.  No threshold is set: the table says what was
measured.  Needs the card: there is no CPU path.  Writes a table (default profiles/scaled_decode.txt) and prints it.

    python tools/scaled_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/scaled_decode.txt]
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
    ap.add_argument("--small", action="store_true", help="a rehearsal at 1/16 of the frame sizes")
    ap.add_argument("--check", type=int, default=1, help="distinct slots compared with the host expectation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_decode.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)

    import compeg_amd as ca
    import reduced_stream as rs
    import scaled_stream as sc
    from tools import synth

    n, distinct, k = args.batch, min(args.distinct, args.batch), 4 if args.small else 1
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    stream = torch.cuda.Stream()
    sets = (("422", 3840 // k, 2160 // k, dict(), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4)),
            ("420", 1920 // k, 1080 // k, dict(allow_sampling=True), lambda w, h, i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4, sampling=(2, 2))))
    lines = [f"scaled (1/2, 1/4) decode against the RGBA decode of the same frames: {n} resident frames ({distinct} distinct) a batch; {gpu.name()}",
             f"rows in turn (RGBA, reduced, scaled 1/2 and 1/4 in both formats, RGBA + pack /2, RGBA + pack /4, RGBA, ...), median of {args.reps} (min .. max);",
             "ms: device events on the stream around the row's calls; out B/frame: bytes the row writes per frame; vs RGBA: the row's median over the RGBA row's",
             f"{'frames':<22} {'row':<28} {'kernel':<13} {'out B/frame':>12} {'ms':>28} {'vs RGBA':>8}"]
    notes = []
    for layout, w, h, kw, make in sets:
        jpegs = [make(w, h, i) for i in range(distinct)]
        images = [ca.ImageData(j, **kw) for j in jpegs]
        hs, vs = images[0].sampling()
        batch = ca.Batch(gpu)
        batch.upload([images[i % distinct] for i in range(n)])
        dests = {}
        for den in (2, 4):
            for format in sc.FORMATS:
                total = ca.scaled_shape(w, h, den, format)[3]
                dests[(den, format)] = (torch.zeros(total * n, dtype=torch.uint8, device="cuda"), total)
        rtotal = ca.reduced_shape(w, h)[3]
        reduced = torch.zeros(rtotal * n, dtype=torch.uint8, device="cuda")
        packed = {}
        for den in (2, 4):
            try:
                _, tbytes = ca.tensor_shape(w, h, "u8", den)
                packed[den] = (torch.zeros(tbytes * n, dtype=torch.uint8, device="cuda"), tbytes)
            except ca.Error as e:   # (an extent the pack's block mean does not divide: the chain row is left out)
                notes.append(f"{layout}: no chain row at /{den}: {e}")
        # the scaled image against the host expectation, on a few of the distinct slots
        same = True
        checked = min(args.check, distinct)
        coefs = [rs.file_coefficients(ca, jpegs[i], **kw) for i in range(checked)]
        for (den, format), (dst, total) in dests.items():
            batch.decode_scaled(dst, den, format, hip_stream=stream.cuda_stream)
            batch.wait()
            for i, (coef, (_, _, _, _, _, dpm, mcus_w, mcus_h), _) in enumerate(coefs):
                want = sc.destination(sc.scaled_planes(coef, den, dpm, hs, vs, mcus_w, mcus_h), w, h, den, hs, vs, format)
                same = same and bool(np.array_equal(dst[i * total:(i + 1) * total].cpu().numpy(), want))
        notes.append(f"{layout}: scaled images equal the host expectation on {checked} slot(s), both scales, both formats: {'yes' if same else 'NO'}")

        def run(kind):
            if kind == "full":
                batch.decode(stream.cuda_stream)
            elif kind == "reduced":
                batch.decode_reduced(reduced, "rgba", hip_stream=stream.cuda_stream)
            elif kind[0] == "chain":
                batch.decode(stream.cuda_stream)
                batch.pack_tensor(packed[kind[1]][0], dtype="u8", downscale=kind[1], hip_stream=stream.cuda_stream)
            else:
                batch.decode_scaled(dests[kind][0], kind[0], kind[1], hip_stream=stream.cuda_stream)

        kinds = ["full", "reduced"] + list(dests) + [("chain", den) for den in packed]
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
            if kind == "full":
                row, out_bytes = "RGBA (Batch.decode)", 4 * w * h
            elif kind == "reduced":
                row, out_bytes = "reduced 1/8 rgba", rtotal
            elif kind[0] == "chain":
                row, out_bytes = f"RGBA + pack_tensor(/{kind[1]}, u8)", 4 * w * h + packed[kind[1]][1]
            else:
                row, out_bytes = f"scaled 1/{kind[0]} {kind[1]}", dests[kind][1]
            lines.append(f"{f'{w}x{h} {layout}':<22} {row:<28} {names[kind]:<13} {out_bytes:>12} "
                         f"{med:>9.3f} ({min(t):.3f} .. {max(t):.3f}) {med / base:>8.3f}")
        del batch, dests, packed, reduced
    lines += notes
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
