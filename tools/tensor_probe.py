"""Tensor output (Batch.pack_tensor) against what a user writes today, on the benchmark's workload.

256 of bench.py's 4K 4:2:2 DRI=4 frames, resident, decoded once.  Per variant (element type, downscale factor):
the pack alone, timed with HIP events on its stream, launch by launch in turn with the eager torch chain on a
zero-copy strided view of the batch's output --

    x[..., :3].permute(0, 3, 1, 2).to(dtype) * scale + bias        (avg_pool2d in front for k > 1; u8: .contiguous())

-- whose last bits may differ (it is a timing baseline only).  Bytes moved by the pack: (4 W H + 3 esize ow oh) N;
the rate as a share of the 8 TB/s of the project's roofline (bench.py: HBM_PEAK_GBS).  Then decode + pack against
decode alone.  Every variant is warmed up first and the clock primed as bench.py does it.  Needs the card: there is
no CPU path.  Writes a table (default profiles/tensor_pack.txt) and prints it.

    python tools/tensor_probe.py [--batch 256] [--distinct 256] [--reps 10] [--out profiles/tensor_pack.txt]
"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
PRIME_SECONDS = 0.08
VARIANTS = (("f16", 1), ("f16", 2), ("f16", 4), ("u8", 1), ("f32", 1))
ESIZE = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class _BatchView:
    """__cuda_array_interface__ of the whole batch output: [N, H, W, 4] u8, images one stride apart, rows one pitch."""

    def __init__(self, batch, n):
        first, second = batch.output(0), batch.output(1 if n > 1 else 0)
        stride = second.ptr - first.ptr if n > 1 else first.pitch * first.height
        self.__cuda_array_interface__ = {"shape": (n, first.height, first.width, 4), "typestr": "|u1", "data": (first.ptr, False),
                                         "strides": (stride, first.pitch, 4, 1), "version": 3}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--distinct", type=int, default=0, help="distinct synthetic frames (0 = one per slot, like bench.py)")
    p.add_argument("--width", type=int, default=3840)
    p.add_argument("--height", type=int, default=2160)
    p.add_argument("--reps", type=int, default=10, help="timed launches per variant, of the pack and of the chain in turn")
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_pack.txt"))
    args = p.parse_args()

    import torch
    import torch.nn.functional as F

    import compeg_amd
    from tools import synth

    if not torch.cuda.is_available():
        raise SystemExit("tensor_probe: no GPU (nothing here is measured without one)")
    n, w, h = args.batch, args.width, args.height
    distinct = min(args.distinct or n, n)
    with ThreadPoolExecutor(args.threads) as ex:
        jpegs = list(ex.map(lambda i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4), range(distinct)))
    gpu = compeg_amd.Gpu.open(0)
    images = [compeg_amd.ImageData(j, copy=False) for j in jpegs]
    batch = compeg_amd.Batch(gpu)
    batch.upload([images[i % distinct] for i in range(n)], host_threads=args.threads)
    stream = torch.cuda.Stream()
    handle = stream.cuda_stream

    def prime():
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < PRIME_SECONDS:
            batch.decode(handle)
            batch.wait()

    prime()
    batch.decode(handle)
    batch.wait()
    view = torch.as_tensor(_BatchView(batch, n), device="cuda")
    assert view.shape == (n, h, w, 4) and view.data_ptr() == batch.output(0).ptr   # zero-copy

    torch_type = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
    lines = [f"tensor output: {n} x {w}x{h} 4:2:2 DRI=4 frames ({distinct} distinct), resident, decoded once; {gpu.name()}",
             f"pack = Batch.pack_tensor alone, HIP events on its stream; chain = eager torch on a zero-copy view of the same output, "
             f"launch by launch in turn; median of {args.reps} (min .. max); bytes = (4 W H + 3 esize ow oh) N; share of {HBM_PEAK_GBS / 1000:.0f} TB/s",
             f"{'variant':<10} {'pack ms':>22} {'GB moved':>9} {'TB/s':>6} {'share':>6} {'chain ms':>24} {'chain/pack':>10}"]
    slower = []
    for dtype, k in VARIANTS:
        ow, oh = w // k, h // k
        scale = [1.0] * 3 if dtype == "u8" else [1.0 / (255.0 * s) for s in STD]
        bias = [0.0] * 3 if dtype == "u8" else [-m / s for m, s in zip(MEAN, STD)]
        dst = torch.empty((n, 3, oh, ow), dtype=torch_type[dtype], device="cuda")
        with torch.cuda.stream(stream):
            ts = torch.tensor(scale, dtype=torch_type[dtype] if dtype != "u8" else torch.float32, device="cuda").view(1, 3, 1, 1)
            tb = torch.tensor(bias, dtype=torch_type[dtype] if dtype != "u8" else torch.float32, device="cuda").view(1, 3, 1, 1)

        def pack():
            batch.pack_tensor(dst, dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=handle)

        def chain():
            x = view[..., :3].permute(0, 3, 1, 2)
            if dtype == "u8":
                return x.contiguous()
            x = x.to(torch_type[dtype])
            if k > 1:
                x = F.avg_pool2d(x, k)
            return x * ts + tb

        with torch.cuda.stream(stream):
            for _ in range(2):   # warm-up of both: code objects, the allocator's blocks
                pack()
                y = chain()
                del y
            stream.synchronize()
            prime()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.reps)]
            for e0, e1, e2 in ev:
                e0.record(stream)
                pack()
                e1.record(stream)
                y = chain()
                e2.record(stream)
                del y
            stream.synchronize()
        t_pack = [a.elapsed_time(b) for a, b, _ in ev]
        t_chain = [b.elapsed_time(c) for _, b, c in ev]
        mp, mc = statistics.median(t_pack), statistics.median(t_chain)
        moved = (4 * w * h + 3 * ESIZE[dtype] * ow * oh) * n
        rate = moved / (mp * 1e-3) / 1e12
        lines.append(f"{dtype + ' k=' + str(k):<10} {mp:8.3f} ({min(t_pack):.3f} .. {max(t_pack):.3f}) {moved / 1e9:9.2f} {rate:6.2f} "
                     f"{100 * rate * 1000 / HBM_PEAK_GBS:5.1f}% {mc:9.3f} ({min(t_chain):.3f} .. {max(t_chain):.3f}) {mc / mp:10.2f}")
        if mp > mc:
            slower.append(f"{dtype} k={k}")
        del dst
        torch.cuda.empty_cache()

    # decode + pack against decode alone (f16, k = 1), alternating; host clock around work that ends in a synchronise
    dst = torch.empty((n, 3, h, w), dtype=torch.float16, device="cuda")
    scale, bias = [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)]
    batch.set_timing(False)
    alone, both = [], []
    prime()
    for _ in range(args.reps):
        t0 = time.perf_counter()
        batch.decode(handle)
        batch.wait()
        alone.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        batch.decode(handle)
        batch.pack_tensor(dst, dtype="f16", scale=scale, bias=bias, hip_stream=handle)
        batch.wait()
        both.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"decode alone {statistics.median(alone):.3f} ms ({min(alone):.3f} .. {max(alone):.3f}); decode + pack f16 k=1 "
                 f"{statistics.median(both):.3f} ms ({min(both):.3f} .. {max(both):.3f}); host clock, submit to synchronise, median of {args.reps}")
    lines.append("pack slower than the chain beside it: " + (", ".join(slower) if slower else "none"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
