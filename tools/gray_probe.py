"""Grayscale decode against its own yardstick: the 4:4:4 kernel on the frames' twins.

256 resident 1920x1080 frames (a few distinct pictures, each in several slots), written by PIL as `L` images with
restart_marker_blocks = 8 and = 5; their twins are the same pictures saved as RGB without subsampling -- R = G = B, so
Cb = Cr = 128 and every chroma data unit is "DC difference 0, EOB": the same luma data units, the same pixels, the same
stores, three times the data units.  Grayscale does a third of the entropy work and writes the same bytes: it must
not be slower than its twin.

In one process: both batches uploaded once; outputs compared once (standard entropy: the twin's chroma units move the
bit positions, which shows in the reference's mode where its reader runs dry); then, in the default entropy mode, the
decodes timed in turn -- twin, grayscale, twin, ... -- after a warm-up and with the clock primed, by the batch's own
HIP events (compeg_batch_timing: kernel time on the stream) and by a host clock from submit to synchronise.  Needs the
card: there is no CPU path.  Writes a table (default profiles/gray_decode.txt) and prints it.

    python tools/gray_probe.py [--batch 256] [--distinct 8] [--reps 20] [--out profiles/gray_decode.txt]
"""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIME_SECONDS = 0.08


def picture(w, h, seed):
    """A smooth scene with texture and noise on it: scans of a camera frame's density."""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 128 + 70 * np.sin(xx / (37.0 + seed)) * np.cos(yy / (53.0 - seed)) + 25 * np.sin((xx + 2 * yy) / 5.0)
    img += rng.normal(0, 6, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, blocks, colour):
    from PIL import Image
    out = io.BytesIO()
    if colour:
        import numpy as np
        Image.fromarray(np.repeat(img[:, :, None], 3, axis=2), "RGB").save(out, "JPEG", quality=85, subsampling=0, restart_marker_blocks=blocks)
    else:
        Image.fromarray(img, "L").save(out, "JPEG", quality=85, restart_marker_blocks=blocks)
    return out.getvalue()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--distinct", type=int, default=8)
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--reps", type=int, default=20, help="timed decodes of each batch, in turn")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "gray_decode.txt"))
    args = p.parse_args()

    import numpy as np

    import compeg_amd as ca

    n, w, h = args.batch, args.width, args.height
    distinct = min(args.distinct, n)
    gpu = ca.Gpu.open(0)   # (fails without a card: nothing here is measured without one)
    lines = [f"grayscale decode against the 4:4:4 kernel on the twins: {n} x {w}x{h} frames ({distinct} distinct), resident; {gpu.name()}",
             f"PIL quality 85; twin = the picture saved as RGB without subsampling; decodes in turn (twin, grayscale, ...), median of {args.reps} (min .. max);",
             "kernel ms: compeg_batch_timing (HIP events on the decode's stream); host ms: submit to synchronise",
             f"{'DRI':>4} {'batch':<10} {'kernel':<13} {'scan MB':>8} {'kernel ms':>26} {'host ms':>26}"]
    verdicts = []
    for blocks in (8, 5):
        pictures = [picture(w, h, s) for s in range(distinct)]
        files = {"grayscale": [encode(img, blocks, False) for img in pictures], "twin 4:4:4": [encode(img, blocks, True) for img in pictures]}
        kw = {"grayscale": dict(allow_grayscale=True), "twin 4:4:4": dict(allow_sampling=True)}
        # the same pixels (standard entropy), checked on the distinct pictures
        check = {}
        for name, js in files.items():
            b = ca.Batch(gpu)
            b.upload([ca.ImageData(j, standard_entropy=True, **kw[name]) for j in js])
            b.decode()
            b.wait()
            check[name] = [b.read_output(i) for i in range(distinct)]
            del b
        same = all(np.array_equal(a, c) for a, c in zip(check["grayscale"], check["twin 4:4:4"]))
        batches = {}
        for name, js in files.items():
            b = ca.Batch(gpu)
            b.upload([ca.ImageData(js[i % distinct], **kw[name]) for i in range(n)])
            batches[name] = b

        def prime():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                for b in batches.values():
                    b.decode()
                    b.wait()

        for b in batches.values():   # warm-up: code objects, the planner's choices
            for _ in range(2):
                b.decode()
                b.wait()
        prime()
        kernel_ms = {name: [] for name in batches}
        host_ms = {name: [] for name in batches}
        for _ in range(args.reps):
            for name in ("twin 4:4:4", "grayscale"):
                b = batches[name]
                b.timing(reset=True)
                t0 = time.perf_counter()
                b.decode()
                b.wait()
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                decodes, total, _, _ = b.timing(reset=True)
                assert decodes == 1
                kernel_ms[name].append(total)
        for name in ("grayscale", "twin 4:4:4"):
            k, t = kernel_ms[name], host_ms[name]
            mb = sum(len(files[name][i % distinct]) for i in range(n)) / 1e6
            lines.append(f"{blocks:>4} {name:<10} {batches[name].last_kernel():<13} {mb:8.1f} {statistics.median(k):10.3f} ({min(k):.3f} .. {max(k):.3f}) "
                         f"{statistics.median(t):10.3f} ({min(t):.3f} .. {max(t):.3f})")
        ratio = statistics.median(kernel_ms["grayscale"]) / statistics.median(kernel_ms["twin 4:4:4"])
        verdicts.append(f"DRI {blocks}: grayscale / twin = {ratio:.3f} (kernel ms); outputs equal under standard entropy: {'yes' if same else 'NO'}"
                        + ("" if ratio <= 1.0 else "  -- grayscale is SLOWER than its twin"))
        del batches
    lines += verdicts
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
