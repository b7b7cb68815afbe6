"""Resized tensor output (Batch.pack_tensor_resized) against what a user writes today.

Resident batches of 4:2:2 DRI=4 frames, decoded once.  Per configuration: the resized pack alone, timed with HIP
events on its stream, launch by launch in turn with the chain a caller of pack_tensor writes --

    Batch.pack_tensor(f32, k)  ->  F.interpolate(mode="bilinear", antialias=False)  ->  * scale + bias  ->  .to(dtype)

(f32 so that nothing is rounded twice; u8: rounded and clamped before the cast) -- whose last bits may differ (it is
a timing baseline only).  The mixed batch has four sizes: its baseline is one such chain per size group, each group a
resident batch of its own, written into its slice of the output.  Every configuration is warmed up first and the
clock primed as bench.py does it.  Needs the card: there is no CPU path.  Writes a table (default
profiles/tensor_resize.txt) and prints it.

    python tools/resize_probe.py [--batch 256] [--distinct 16] [--reps 10] [--out profiles/tensor_resize.txt]

The antialias arm (--antialias; default table profiles/tensor_resize_antialias.txt): resident batches of 1920x1080 and
of 3840x2160 -> 224x224 in f16, at k = 1 and at the largest k that leaves both axes shrinking.  Per configuration,
launch by launch in turn and by HIP events on one stream: the antialiased pack, the plain bilinear pack at the same
shapes, and the decode of the same batch, which is what the pack follows in a pipeline.

The regions arm (--regions; default table profiles/tensor_regions.txt), the same method: Batch.pack_tensor_regions with
dst the whole output beside pack_tensor_resized of the same launch (the work is identical); the letterbox of 4K into
640x640 beside the chain it replaces, a resized pack to 640x360 into a temporary and torch.nn.functional.pad; and 1024
crops of 128x128 out of 16 4K frames in one call beside 1024 single Decoder.pack_tensor_resized calls.

The filtered arm (--filtered; default table profiles/tensor_filtered.txt), the same method: Batch.pack_tensor_filtered
with each of the four kernels, whole frames of 1080p and of 4K -> 224x224 in f16 at k = 1 and 4K at k = 8, beside the
antialiased Batch.pack_tensor_regions of the same regions (the same arithmetic as the triangle arm: a lane per element
against a lane per band of rows) and the decode of the same batch.

The oriented arm (--oriented; default table profiles/tensor_oriented.txt), the same method: Batch.pack_tensor_oriented of
whole frames -> 224x224, bicubic, k = 1, at the orientations 1, 2 and 6, beside Batch.pack_tensor_filtered and the chains
a user writes without it: the filtered pack into a temporary, then torch.rot90(t, -1, (2, 3)).contiguous() for
orientation 6, t.flip(3) for orientation 2.

The channels-last arm (--nhwc; default table profiles/tensor_nhwc.txt), the same method: Batch.pack_tensor_nhwc with 3 and
with 4 channels beside the planar Batch.pack_tensor_oriented and the chain a user writes without it -- the planar pack into
a temporary, then .contiguous(memory_format=torch.channels_last) --, to 224x224 and, where the stores are not small beside
the loads, 1080p -> 1920x1080 without a resize.

The luma arm (--luma; default table profiles/tensor_luma.txt), the same method: Batch.pack_tensor_luma (BT.601) beside the
three-plane Batch.pack_tensor_oriented of the same launch and the chain a user writes without it -- the oriented pack into a
temporary, then tmp[:, :1].contiguous() --, to 224x224 from 1080p (orientations 1 and 6) and from 4K, and 1080p ->
1920x1080 without a resize on colour 4:2:2 frames and on grayscale frames (PIL's L files, restart_marker_blocks = 8).
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

PRIME_SECONDS = 0.08
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (name, ((width, height), ...) -- the batch's slots split evenly between them --, output size, element type, k)
CONFIGS = (("4K -> 224x224 f16 k=8", ((3840, 2160),), (224, 224), "f16", 8),
           ("4K -> 224x224 f16 k=1", ((3840, 2160),), (224, 224), "f16", 1),
           ("1080p -> 640x640 f16 k=1", ((1920, 1080),), (640, 640), "f16", 1),
           ("960x720 -> 224x224 u8 k=2", ((960, 720),), (224, 224), "u8", 2),
           ("mixed -> 224x224 f16 k=1", ((1920, 1080), (1280, 720), (960, 720), (640, 360)), (224, 224), "f16", 1))


# the antialias arm: (name, (width, height), output size, element type, k)
ANTIALIAS_CONFIGS = (("1080p -> 224x224 f16 k=1", (1920, 1080), (224, 224), "f16", 1),
                     ("1080p -> 224x224 f16 k=4", (1920, 1080), (224, 224), "f16", 4),
                     ("4K -> 224x224 f16 k=1", (3840, 2160), (224, 224), "f16", 1),
                     ("4K -> 224x224 f16 k=8", (3840, 2160), (224, 224), "f16", 8))


def antialias_arm(args, torch, compeg_amd, images_of, resident, gpu, stream):
    """The table of the antialias arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import antialias_reference as ar   # the header's contract in numpy
    n, handle = args.batch, stream.cuda_stream
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-m / s for m, s in zip(MEAN, STD)]
    lines = [f"antialiased resized tensor output: {n} resident 4:2:2 DRI=4 frames per configuration; {gpu.name()}",
             f"antialias = Batch.pack_tensor_resized(antialias=True), bilinear = the same call without the flag, decode = Batch.decode of the same "
             f"batch; HIP events on one stream, launch by launch in turn; median of {args.reps} (min .. max)",
             f"{'configuration':<26} {'antialias ms':>26} {'bilinear ms':>24} {'decode ms':>24} {'antialias/decode':>16}"]
    dearer = []
    for name, (w, h), (ow, oh), dtype, k in ANTIALIAS_CONFIGS:
        items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        dst = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")
        plain = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")

        def pack(out, antialias):
            batch.pack_tensor_resized(out, (ow, oh), dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=handle, antialias=antialias)

        with torch.cuda.stream(stream):
            for _ in range(2):   # warm-up: code objects, the staging blocks
                pack(dst, True)
                pack(plain, False)
                batch.decode(handle)
            stream.synchronize()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.reps)]
            for e in ev:
                e[0].record(stream)
                pack(dst, True)
                e[1].record(stream)
                pack(plain, False)
                e[2].record(stream)
                batch.decode(handle)
                e[3].record(stream)
            stream.synchronize()
        t = [[e[i].elapsed_time(e[i + 1]) for e in ev] for i in range(3)]
        med = [statistics.median(x) for x in t]
        # (slot 0 against the contract on the host: what is timed is what the header defines)
        wrong = int((ar.expected(batch.read_output(0), (ow, oh), k, dtype, scale, bias) != dst[0].cpu().numpy()).sum())
        cells = " ".join(f"{m:9.3f} ({min(x):.3f} .. {max(x):.3f})" for m, x in zip(med, t))
        lines.append(f"{name:<26} {cells} {med[0] / med[2]:16.2f}   slot 0: {wrong} elements off the contract")
        if med[0] > med[2]:
            dearer.append(name)
        del dst, plain, batch
        torch.cuda.empty_cache()
    lines.append("antialiased pack dearer than the decode it follows: " + ("; ".join(dearer) if dearer else "none"))
    return "\n".join(lines) + "\n"


# the regions arm, dst whole: (name, (width, height), output size, antialias)
REGION_WHOLE_CONFIGS = (("1080p -> 224x224 bilinear", (1920, 1080), (224, 224), False),
                        ("1080p -> 224x224 antialias", (1920, 1080), (224, 224), True),
                        ("4K -> 224x224 bilinear", (3840, 2160), (224, 224), False),
                        ("4K -> 224x224 antialias", (3840, 2160), (224, 224), True))
GREY = (114.0, 114.0, 114.0)


def _timed_in_turn(torch, stream, reps, prime, arms):
    """Every arm launched in turn, `reps` times, between HIP events on `stream`: a list of `reps` times (ms) per arm.  The
    order of the arms turns round from one repetition to the next, so that no arm is always the one behind another; and
    one untimed round stands between the priming and the first timed one, whose first launch is 0.1 to 0.3 ms slower
    whichever arm it is."""
    with torch.cuda.stream(stream):
        for _ in range(2):   # warm-up: code objects, the staging blocks, the allocator's blocks
            for arm in arms:
                arm()
        stream.synchronize()
        prime()
        for arm in arms:
            arm()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(arms))] for _ in range(reps)]
        for r, e in enumerate(ev):
            for i in range(len(arms)):
                a = (i + r) % len(arms)
                e[2 * a].record(stream)
                arms[a]()
                e[2 * a + 1].record(stream)
        stream.synchronize()
    return [[e[2 * a].elapsed_time(e[2 * a + 1]) for e in ev] for a in range(len(arms))]


def _cell(x):
    return f"{statistics.median(x):9.3f} ({min(x):.3f} .. {max(x):.3f})"


def _gap(a, b):
    """Whether the medians of two rows lie further apart than the rows' own min-to-max spread."""
    return abs(statistics.median(a) - statistics.median(b)) > max(max(a) - min(a), max(b) - min(b))


def regions_arm(args, torch, F, compeg_amd, images_of, resident, gpu, stream):
    """The table of the regions arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import region_reference as gr   # the header's contract in numpy
    n, handle = args.batch, stream.cuda_stream
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-m / s for m, s in zip(MEAN, STD)]

    def primer(batch):
        def prime():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()
        return prime

    lines = [f"region tensor output: resident 4:2:2 DRI=4 frames, decoded once; {gpu.name()}",
             f"HIP events on one stream, the arms of a row launch by launch in turn, their order turning round from one repetition to the next, one "
             f"untimed round in front; median of {args.reps} (min .. max); f16, k = 1",
             "",
             f"dst whole: {n} frames, regions = Batch.pack_tensor_regions with every dst the whole output, resized = Batch.pack_tensor_resized",
             f"{'configuration':<28} {'regions ms':>26} {'resized ms':>26} {'regions/resized':>15}"]
    gaps = []
    for name, (w, h), (ow, oh), antialias in REGION_WHOLE_CONFIGS:
        items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        a = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")
        b = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")
        whole = [(i, None, None) for i in range(n)]
        kw = dict(dtype="f16", scale=scale, bias=bias, hip_stream=handle, antialias=antialias)
        t = _timed_in_turn(torch, stream, args.reps, primer(batch),
                           [lambda: batch.pack_tensor_regions(a, (ow, oh), whole, pad=GREY, **kw), lambda: batch.pack_tensor_resized(b, (ow, oh), **kw)])
        filt = "antialias" if antialias else "bilinear"
        wrong = int((gr.expected(batch.read_output(0), (ow, oh), 1, "f16", scale, bias, "rgb", filt) != a[0].cpu().numpy()).sum())
        equal = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
        lines.append(f"{name:<28} {_cell(t[0])} {_cell(t[1])} {statistics.median(t[0]) / statistics.median(t[1]):15.3f}   slot 0: {wrong} elements off the "
                     f"contract; all slots equal to resized: {equal}")
        print(lines[-1], file=sys.stderr, flush=True)   # (progress: the table itself is printed at the end)
        if _gap(t[0], t[1]):
            gaps.append(name)
        del a, b, batch
        torch.cuda.empty_cache()
    lines.append("rows whose medians lie further apart than their own min-to-max spread: " + ("; ".join(gaps) if gaps else "none"))

    # the letterbox: 4K fitted into 640x640; a uniform scale, so that the chain's one pad value is the contract's
    (w, h), (ow, oh) = (3840, 2160), (640, 640)
    dx, dy, dw, dh = compeg_amd.region_fit((w, h), (ow, oh))
    items = images_of(w, h)
    batch = resident([items[i % len(items)] for i in range(n)])
    uniform, zero = [1.0 / 255.0] * 3, [0.0] * 3
    lines += ["", f"letterbox: {n} 4K frames -> 640x640, inner rectangle ({dx}, {dy}, {dw}, {dh}), pad 114, scale 1/255; chain = pack_tensor_resized to "
              f"{dw}x{dh} into a temporary, then torch.nn.functional.pad",
              f"{'configuration':<28} {'regions ms':>26} {'chain ms':>26} {'chain/regions':>15}"]
    for antialias in (False, True):
        a = torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda")
        tmp = torch.empty((n, 3, dh, dw), dtype=torch.float16, device="cuda")
        box = [(i, None, (dx, dy, dw, dh)) for i in range(n)]
        kw = dict(dtype="f16", scale=uniform, bias=zero, hip_stream=handle, antialias=antialias)
        kept = {}

        def chain():
            batch.pack_tensor_resized(tmp, (dw, dh), **kw)
            kept["b"] = F.pad(tmp, (dx, ow - dx - dw, dy, oh - dy - dh), value=114.0 / 255.0)

        t = _timed_in_turn(torch, stream, args.reps, primer(batch), [lambda: batch.pack_tensor_regions(a, (ow, oh), box, pad=GREY, **kw), chain])
        filt = "antialias" if antialias else "bilinear"
        wrong = int((gr.expected(batch.read_output(0), (ow, oh), 1, "f16", uniform, zero, "rgb", filt, None, (dx, dy, dw, dh), GREY) != a[0].cpu().numpy()).sum())
        worst = float((a.float() - kept["b"].float()).abs().max())
        lines.append(f"{'4K -> 640x640 ' + filt:<28} {_cell(t[0])} {_cell(t[1])} {statistics.median(t[1]) / statistics.median(t[0]):15.2f}   slot 0: {wrong} "
                     f"elements off the contract; max |regions - chain| {worst:.4g}")
        print(lines[-1], file=sys.stderr, flush=True)
        del a, tmp, kept
        torch.cuda.empty_cache()
    del batch
    torch.cuda.empty_cache()

    # the crop list: 1024 crops of 128x128 out of 16 4K frames, one call against one call per crop
    frames, crops, (cw, ch), (ow, oh) = 16, 1024, (128, 128), (224, 224)
    items = [images_of(w, h)[i % len(images_of(w, h))] for i in range(frames)]
    batch = resident(items)
    decoders = []
    for item in items:
        dec = compeg_amd.Decoder(gpu)
        dec.decode_blocking(item)
        decoders.append(dec)
    # (a fixed scatter: crop c comes from frame c % 16, its origin steps through the frame)
    rects = [((c * 397) % (w - cw), (c * 211) % (h - ch), cw, ch) for c in range(crops)]
    regions = [(c % frames, rects[c], None) for c in range(crops)]
    lines += ["", f"crop list: {crops} crops of {cw}x{ch} out of {frames} 4K frames -> 224x224; regions = one Batch.pack_tensor_regions, singles = {crops} "
              f"Decoder.pack_tensor_resized calls on {frames} decoders that hold the same frames",
              f"{'configuration':<28} {'regions ms':>26} {'singles ms':>26} {'singles/regions':>15}"]
    for antialias in (False, True):
        a = torch.empty((crops, 3, oh, ow), dtype=torch.float16, device="cuda")
        b = torch.empty((crops, 3, oh, ow), dtype=torch.float16, device="cuda")
        kw = dict(dtype="f16", scale=scale, bias=bias, hip_stream=handle, antialias=antialias)

        def singles():
            for c in range(crops):
                decoders[c % frames].pack_tensor_resized(b[c], (ow, oh), crop=rects[c], **kw)

        t = _timed_in_turn(torch, stream, args.reps, primer(batch), [lambda: batch.pack_tensor_regions(a, (ow, oh), regions, pad=GREY, **kw), singles])
        filt = "antialias" if antialias else "bilinear"
        wrong = int((gr.expected(batch.read_output(0), (ow, oh), 1, "f16", scale, bias, "rgb", filt, rects[0]) != a[0].cpu().numpy()).sum())
        equal = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
        lines.append(f"{'128x128 -> 224x224 ' + filt:<28} {_cell(t[0])} {_cell(t[1])} {statistics.median(t[1]) / statistics.median(t[0]):15.2f}   slot 0: {wrong} "
                     f"elements off the contract; all slots equal to the singles: {equal}")
        print(lines[-1], file=sys.stderr, flush=True)
        del a, b
        torch.cuda.empty_cache()
    return "\n".join(lines) + "\n"


# the filtered arm: (name, (width, height), output size, k)
FILTERED_CONFIGS = (("1080p -> 224x224 f16 k=1", (1920, 1080), (224, 224), 1),
                    ("4K -> 224x224 f16 k=1", (3840, 2160), (224, 224), 1),
                    ("4K -> 224x224 f16 k=8", (3840, 2160), (224, 224), 8))


def filtered_arm(args, torch, compeg_amd, images_of, resident, gpu, stream):
    """The table of the filtered arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import filter_reference as fr   # the header's contracts in numpy
    n, handle = args.batch, stream.cuda_stream
    scale = [1.0 / (255.0 * s) for s in STD]
    bias = [-m / s for m, s in zip(MEAN, STD)]
    kernels = list(compeg_amd.FILTER_KERNELS)
    lines = [f"filtered tensor output: {n} resident 4:2:2 DRI=4 frames per configuration, decoded once; {gpu.name()}; library {os.path.relpath(compeg_amd.LIB_PATH, ROOT)}",
             f"box .. lanczos3 = Batch.pack_tensor_filtered of whole frames; antialias = Batch.pack_tensor_regions(antialias=True) of the same regions "
             f"(triangle's arithmetic, a lane per element); decode = Batch.decode of the same batch",
             f"HIP events on one stream, the arms of a configuration launch by launch in turn, their order turning round from one repetition to the "
             f"next, one untimed round in front; median of {args.reps} (min .. max), ms"]
    verdicts = []
    for name, (w, h), (ow, oh), k in FILTERED_CONFIGS:
        items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        whole = [(i, None, None) for i in range(n)]
        out = {key: torch.empty((n, 3, oh, ow), dtype=torch.float16, device="cuda") for key in kernels + ["antialias"]}
        kw = dict(dtype="f16", downscale=k, scale=scale, bias=bias, hip_stream=handle)

        def primer():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()

        arms = [(lambda key=key: batch.pack_tensor_filtered(out[key], (ow, oh), whole, kernel=key, **kw)) for key in kernels]
        arms.append(lambda: batch.pack_tensor_regions(out["antialias"], (ow, oh), whole, antialias=True, **kw))
        arms.append(lambda: batch.decode(handle))
        t = _timed_in_turn(torch, stream, args.reps, primer, arms)
        rgba = batch.read_output(0)
        lines += ["", name]
        for key, row in zip(kernels, t):
            wrong = int((fr.expected(rgba, (ow, oh), k, "f16", scale, bias, "rgb", key) != out[key][0].cpu().numpy()).sum())
            lines.append(f"  {key:<10} {_cell(row)}   slot 0: {wrong} elements off the contract")
        equal = bool(torch.equal(out["triangle"].view(torch.int16), out["antialias"].view(torch.int16)))
        lines.append(f"  {'antialias':<10} {_cell(t[4])}   all slots equal to triangle: {equal}")
        lines.append(f"  {'decode':<10} {_cell(t[5])}")
        tri, old = t[1], t[4]
        ratio = statistics.median(old) / statistics.median(tri)
        verdict = ("faster" if statistics.median(tri) < statistics.median(old) else "slower") if _gap(tri, old) else "within the rows' own spread"
        lines.append(f"  triangle in bands against the antialiased pack: antialias/triangle {ratio:.2f}, {verdict}")
        verdicts.append(f"{name}: {ratio:.2f} ({verdict})")
        print("\n".join(lines[-9:]), file=sys.stderr, flush=True)   # (progress: the table itself is printed at the end)
        del out, batch
        torch.cuda.empty_cache()
    lines += ["", "antialias/triangle: " + "; ".join(verdicts)]
    return "\n".join(lines) + "\n"


# the oriented arm: (name, (width, height), element type, orientations)
ORIENTED_CONFIGS = (("1080p -> 224x224 f16 k=1", (1920, 1080), "f16", (1, 2, 6)),
                    ("4K -> 224x224 f16 k=1", (3840, 2160), "f16", (1, 2, 6)),
                    ("1080p -> 224x224 u8 k=1", (1920, 1080), "u8", (6,)),      # runs of 8 bytes
                    ("1080p -> 224x224 f32 k=1", (1920, 1080), "f32", (6,)))    # runs of 32 bytes


def oriented_arm(args, torch, compeg_amd, images_of, resident, gpu, stream):
    """The table of the oriented arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orient_reference as orf   # the header's contract in numpy
    n, handle, (ow, oh) = args.batch, stream.cuda_stream, (224, 224)
    torch_type = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
    lines = [f"oriented tensor output: {n} resident 4:2:2 DRI=4 frames per configuration, decoded once; {gpu.name()}; library {os.path.relpath(compeg_amd.LIB_PATH, ROOT)}",
             "filtered = Batch.pack_tensor_filtered of whole frames, bicubic; o=N = Batch.pack_tensor_oriented of the same regions at orientation N; "
             "chain 6 = the filtered pack into a temporary, then torch.rot90(t, -1, (2, 3)).contiguous(); chain 2 = the same, then t.flip(3)",
             f"HIP events on one stream, the arms of a configuration launch by launch in turn, their order turning round from one repetition to the "
             f"next, one untimed round in front; median of {args.reps} (min .. max), ms"]
    verdicts = []
    for name, (w, h), dtype, orientations in ORIENTED_CONFIGS:
        items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        whole = [(i, None, None) for i in range(n)]
        scale = [1.0] * 3 if dtype == "u8" else [1.0 / (255.0 * s) for s in STD]
        bias = [0.0] * 3 if dtype == "u8" else [-m / s for m, s in zip(MEAN, STD)]
        kw = dict(kernel="bicubic", dtype=dtype, scale=scale, bias=bias, hip_stream=handle)
        keys = ["filtered"] + [f"o={o}" for o in orientations] + [f"chain {o}" for o in orientations if o != 1]
        out = {key: torch.empty((n, 3, oh, ow), dtype=torch_type[dtype], device="cuda") for key in keys + ["tmp"]}

        def primer():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()

        def chain(o):
            batch.pack_tensor_filtered(out["tmp"], (ow, oh), whole, **kw)
            out[f"chain {o}"] = torch.rot90(out["tmp"], -1, (2, 3)).contiguous() if o == 6 else out["tmp"].flip(3)

        arms = [lambda: batch.pack_tensor_filtered(out["filtered"], (ow, oh), whole, **kw)]
        arms += [(lambda o=o: batch.pack_tensor_oriented(out[f"o={o}"], (ow, oh), whole, orientation=o, **kw)) for o in orientations]
        arms += [(lambda o=o: chain(o)) for o in orientations if o != 1]
        t = dict(zip(keys, _timed_in_turn(torch, stream, args.reps, primer, arms)))
        rgba = batch.read_output(0)
        lines += ["", name]
        for key in keys:
            o = 1 if key == "filtered" else int(key.split("=")[-1].split()[-1])
            note = ""
            if not key.startswith("chain"):
                wrong = int((orf.expected(rgba, (ow, oh), 1, dtype, scale, bias, "rgb", "bicubic", o=o) != out[key][0].cpu().numpy()).sum())
                note = f"   slot 0: {wrong} elements off the contract"
            else:
                note = f"   all slots equal to o={o}: {bool(torch.equal(out[key], out[f'o={o}']))}"
            lines.append(f"  {key:<10} {_cell(t[key])}{note}")
        for o in orientations:
            other = "filtered" if o != 6 else "chain 6"
            a, b = t[f"o={o}"], t[other]
            ratio = statistics.median(a) / statistics.median(b)
            verdict = ("faster" if statistics.median(a) < statistics.median(b) else "slower") if _gap(a, b) else "within the rows' own spread"
            lines.append(f"  o={o} against {other}: {ratio:.2f}, {verdict}")
            verdicts.append(f"{name}: o={o}/{other} {ratio:.2f} ({verdict})")
        print("\n".join(lines[-(len(keys) + len(orientations) + 1):]), file=sys.stderr, flush=True)   # (progress: the table itself is printed at the end)
        del out, batch
        torch.cuda.empty_cache()
    lines += [""] + verdicts
    return "\n".join(lines) + "\n"


# the channels-last arm: (name, (width, height), (ow, oh), kernel, element type, orientation)
NHWC_CONFIGS = (("1080p -> 224x224 bicubic f16 o=1", (1920, 1080), (224, 224), "bicubic", "f16", 1),
                ("1080p -> 224x224 bicubic f16 o=6", (1920, 1080), (224, 224), "bicubic", "f16", 6),
                ("4K -> 224x224 bicubic f16 o=1", (3840, 2160), (224, 224), "bicubic", "f16", 1),
                ("4K -> 224x224 bicubic f16 o=6", (3840, 2160), (224, 224), "bicubic", "f16", 6),
                ("1080p -> 224x224 bicubic u8 o=6", (1920, 1080), (224, 224), "bicubic", "u8", 6),
                ("1080p -> 224x224 bicubic f32 o=6", (1920, 1080), (224, 224), "bicubic", "f32", 6),
                ("1080p -> 1920x1080 triangle u8 o=1", (1920, 1080), (1920, 1080), "triangle", "u8", 1))   # no resize: the stores are not small


def nhwc_arm(args, torch, compeg_amd, images_of, resident, gpu, stream):
    """The table of the channels-last arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nhwc_reference as nr   # the header's contract in numpy
    n, handle = args.batch, stream.cuda_stream
    torch_type = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
    lines = [f"channels-last tensor output: {n} resident 4:2:2 DRI=4 frames per configuration, decoded once; {gpu.name()}; library {os.path.relpath(compeg_amd.LIB_PATH, ROOT)}",
             "planar = Batch.pack_tensor_oriented of whole frames into [N, 3, oh, ow]; nhwc3 / nhwc4 = Batch.pack_tensor_nhwc of the same regions into "
             "[N, oh, ow, 3] / [N, oh, ow, 4] (fill 255 for u8, 1 otherwise); chain = the planar pack into a temporary, then "
             ".contiguous(memory_format=torch.channels_last)",
             f"HIP events on one stream, the arms of a configuration launch by launch in turn, their order turning round from one repetition to the "
             f"next, one untimed round in front; median of {args.reps} (min .. max), ms"]
    verdicts = []
    keys = ["planar", "nhwc3", "nhwc4", "chain"]
    for name, (w, h), (ow, oh), kernel, dtype, o in NHWC_CONFIGS:
        items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        whole = [(i, None, None) for i in range(n)]
        scale = [1.0] * 3 if dtype == "u8" else [1.0 / (255.0 * s) for s in STD]
        bias = [0.0] * 3 if dtype == "u8" else [-m / s for m, s in zip(MEAN, STD)]
        fill = 255.0 if dtype == "u8" else 1.0
        kw = dict(orientation=o, kernel=kernel, dtype=dtype, scale=scale, bias=bias, hip_stream=handle)
        out = {key: torch.empty((n, 3, oh, ow), dtype=torch_type[dtype], device="cuda") for key in ("planar", "tmp")}
        out["nhwc3"] = torch.empty((n, oh, ow, 3), dtype=torch_type[dtype], device="cuda")
        out["nhwc4"] = torch.empty((n, oh, ow, 4), dtype=torch_type[dtype], device="cuda")

        def primer():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()

        def chain():
            batch.pack_tensor_oriented(out["tmp"], (ow, oh), whole, **kw)
            out["chain"] = out["tmp"].contiguous(memory_format=torch.channels_last)

        arms = [lambda: batch.pack_tensor_oriented(out["planar"], (ow, oh), whole, **kw),
                lambda: batch.pack_tensor_nhwc(out["nhwc3"], (ow, oh), whole, channels=3, **kw),
                lambda: batch.pack_tensor_nhwc(out["nhwc4"], (ow, oh), whole, channels=4, fill=fill, **kw), chain]
        t = dict(zip(keys, _timed_in_turn(torch, stream, args.reps, primer, arms)))
        planar = nr.orf.expected(batch.read_output(0), (ow, oh), 1, dtype, scale, bias, "rgb", kernel, o=o)
        wrong = {"planar": int((planar != out["planar"][0].cpu().numpy()).sum()),
                 "nhwc3": int((nr.channels_last(planar) != out["nhwc3"][0].cpu().numpy()).sum()),
                 "nhwc4": int((nr.channels_last(planar, 4, fill, dtype) != out["nhwc4"][0].cpu().numpy()).sum())}
        lines += ["", name]
        for key in keys:
            note = (f"   slot 0: {wrong[key]} elements off the contract" if key != "chain" else
                    f"   all slots equal to nhwc3: {bool(torch.equal(out['chain'].permute(0, 2, 3, 1), out['nhwc3']))}")
            lines.append(f"  {key:<8} {_cell(t[key])}{note}")
        for key in ("nhwc3", "nhwc4"):
            for other in ("chain", "planar"):
                a, b = t[key], t[other]
                ratio = statistics.median(a) / statistics.median(b)
                verdict = ("faster" if statistics.median(a) < statistics.median(b) else "slower") if _gap(a, b) else "within the rows' own spread"
                lines.append(f"  {key} against {other}: {ratio:.2f}, {verdict}")
                verdicts.append(f"{name}: {key}/{other} {ratio:.2f} ({verdict})")
        print("\n".join(lines[-(len(keys) + 5):]), file=sys.stderr, flush=True)   # (progress: the table itself is printed at the end)
        del out, batch
        torch.cuda.empty_cache()
    lines += [""] + verdicts
    return "\n".join(lines) + "\n"


# the luma arm: (name, (width, height), output size, kernel, element type, orientation, grayscale frames)
LUMA_CONFIGS = (("1080p -> 224x224 bicubic f16 o=1", (1920, 1080), (224, 224), "bicubic", "f16", 1, False),
                ("1080p -> 224x224 bicubic f16 o=6", (1920, 1080), (224, 224), "bicubic", "f16", 6, False),
                ("4K -> 224x224 bicubic f16 o=1", (3840, 2160), (224, 224), "bicubic", "f16", 1, False),
                ("1080p -> 1920x1080 triangle u8 o=1, colour 4:2:2", (1920, 1080), (1920, 1080), "triangle", "u8", 1, False),
                ("1080p -> 1920x1080 triangle u8 o=1, grayscale", (1920, 1080), (1920, 1080), "triangle", "u8", 1, True))


def luma_arm(args, torch, compeg_amd, images_of, resident, gpu, stream):
    """The table of the luma arm, as text."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import luma_reference as lr   # the header's contract in numpy
    from tools import gray_probe
    n, handle = args.batch, stream.cuda_stream
    torch_type = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
    lines = [f"luma tensor output: {n} resident frames per configuration (4:2:2 DRI=4, or grayscale), decoded once; {gpu.name()}; library "
             f"{os.path.relpath(compeg_amd.LIB_PATH, ROOT)}",
             "luma = Batch.pack_tensor_luma (BT.601) of whole frames into [N, 1, oh, ow]; planes = Batch.pack_tensor_oriented of the same regions into "
             "[N, 3, oh, ow]; chain = the oriented pack into a temporary, then tmp[:, :1].contiguous()",
             f"HIP events on one stream, the arms of a configuration launch by launch in turn, their order turning round from one repetition to the "
             f"next, one untimed round in front; median of {args.reps} (min .. max), ms"]
    verdicts = []
    keys = ["luma", "planes", "chain"]
    for name, (w, h), (ow, oh), kernel, dtype, o, gray in LUMA_CONFIGS:
        if gray:
            count = min(args.distinct, n, 8)
            files = [gray_probe.encode(gray_probe.picture(w, h, seed), 8, False) for seed in range(count)]
            items = [compeg_amd.ImageData(j, allow_grayscale=True) for j in files]
        else:
            items = images_of(w, h)
        batch = resident([items[i % len(items)] for i in range(n)])
        whole = [(i, None, None) for i in range(n)]
        scale, bias = (1.0, 0.0) if dtype == "u8" else (1.0 / (255.0 * STD[0]), -MEAN[0] / STD[0])
        kw = dict(orientation=o, kernel=kernel, dtype=dtype, hip_stream=handle)
        out = {"luma": torch.empty((n, 1, oh, ow), dtype=torch_type[dtype], device="cuda")}
        out.update({key: torch.empty((n, 3, oh, ow), dtype=torch_type[dtype], device="cuda") for key in ("planes", "tmp")})

        def primer():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                batch.decode(handle)
                batch.wait()

        def chain():
            batch.pack_tensor_oriented(out["tmp"], (ow, oh), whole, scale=[scale] * 3, bias=[bias] * 3, **kw)
            out["chain"] = out["tmp"][:, :1].contiguous()

        arms = [lambda: batch.pack_tensor_luma(out["luma"], (ow, oh), whole, weights="bt601", scale=scale, bias=bias, **kw),
                lambda: batch.pack_tensor_oriented(out["planes"], (ow, oh), whole, scale=[scale] * 3, bias=[bias] * 3, **kw), chain]
        t = dict(zip(keys, _timed_in_turn(torch, stream, args.reps, primer, arms)))
        rgba = batch.read_output(0)
        want = lr.expected(rgba, (ow, oh), 1, dtype, scale, bias, "bt601", kernel, o=o)
        planes = lr.orf.expected(rgba, (ow, oh), 1, dtype, [scale] * 3, [bias] * 3, "rgb", kernel, o=o)
        wrong = {"luma": int((want != out["luma"][0, 0].cpu().numpy()).sum()), "planes": int((planes != out["planes"][0].cpu().numpy()).sum()),
                 "chain": int((planes[:1] != out["chain"][0].cpu().numpy()).sum())}
        lines += ["", name]
        for key in keys:
            lines.append(f"  {key:<8} {_cell(t[key])}   slot 0: {wrong[key]} elements off the contract")
        if gray:
            lines.append(f"  grayscale frames: luma equal to plane 0 of planes in every slot: {bool(torch.equal(out['luma'][:, 0], out['planes'][:, 0]))};"
                         f" R = G = B in slot 0: {bool(np.array_equal(rgba[..., 0], rgba[..., 1]) and np.array_equal(rgba[..., 0], rgba[..., 2]))}")
        for other in ("planes", "chain"):
            a, b = t["luma"], t[other]
            ratio = statistics.median(a) / statistics.median(b)
            verdict = ("faster" if statistics.median(a) < statistics.median(b) else "slower") if _gap(a, b) else "within the rows' own spread"
            lines.append(f"  luma against {other}: {ratio:.2f}, {verdict}")
            verdicts.append(f"{name}: luma/{other} {ratio:.2f} ({verdict})")
        print("\n".join(lines[-(len(keys) + 4 + gray):]), file=sys.stderr, flush=True)   # (progress: the table itself is printed at the end)
        del out, batch
        torch.cuda.empty_cache()
    lines += [""] + verdicts
    return "\n".join(lines) + "\n"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--distinct", type=int, default=16, help="distinct synthetic frames per size (timings do not depend on the content)")
    p.add_argument("--reps", type=int, default=10, help="timed launches per configuration, of the pack and of the chain in turn")
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--out", default=None, help="default: profiles/tensor_resize.txt, or profiles/tensor_resize_antialias.txt with --antialias")
    p.add_argument("--antialias", action="store_true", help="the antialias arm instead of the table against the chain")
    p.add_argument("--regions", action="store_true", help="the regions arm (Batch.pack_tensor_regions) instead; default table profiles/tensor_regions.txt")
    p.add_argument("--filtered", action="store_true", help="the filtered arm (Batch.pack_tensor_filtered) instead; default table profiles/tensor_filtered.txt")
    p.add_argument("--oriented", action="store_true", help="the oriented arm (Batch.pack_tensor_oriented) instead; default table profiles/tensor_oriented.txt")
    p.add_argument("--nhwc", action="store_true", help="the channels-last arm (Batch.pack_tensor_nhwc) instead; default table profiles/tensor_nhwc.txt")
    p.add_argument("--luma", action="store_true", help="the luma arm (Batch.pack_tensor_luma) instead; default table profiles/tensor_luma.txt")
    args = p.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "tensor_luma.txt" if args.luma else "tensor_nhwc.txt" if args.nhwc else "tensor_oriented.txt" if args.oriented else "tensor_filtered.txt" if args.filtered else "tensor_regions.txt" if args.regions else
                                "tensor_resize_antialias.txt" if args.antialias else "tensor_resize.txt")

    import torch
    import torch.nn.functional as F

    import compeg_amd
    from tools import synth

    if not torch.cuda.is_available():
        raise SystemExit("resize_probe: no GPU (nothing here is measured without one)")
    n = args.batch
    gpu = compeg_amd.Gpu.open(0)
    stream = torch.cuda.Stream()
    handle = stream.cuda_stream
    torch_type = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
    made = {}

    def images_of(w, h):
        if (w, h) not in made:
            count = min(args.distinct, n)
            with ThreadPoolExecutor(args.threads) as ex:
                jpegs = list(ex.map(lambda i: synth.make_jpeg(w, h, seed=0xC0FFEE + i, quality=85, ri=4), range(count)))
            made[(w, h)] = [compeg_amd.ImageData(j, copy=False) for j in jpegs], jpegs
        return made[(w, h)][0]

    def resident(items):
        batch = compeg_amd.Batch(gpu)
        batch.upload(items, host_threads=args.threads)
        batch.decode(handle)
        batch.wait()
        return batch

    if args.antialias or args.regions or args.filtered or args.oriented or args.nhwc or args.luma:
        text = (luma_arm(args, torch, compeg_amd, images_of, resident, gpu, stream) if args.luma else
                nhwc_arm(args, torch, compeg_amd, images_of, resident, gpu, stream) if args.nhwc else
                oriented_arm(args, torch, compeg_amd, images_of, resident, gpu, stream) if args.oriented else
                filtered_arm(args, torch, compeg_amd, images_of, resident, gpu, stream) if args.filtered else
                regions_arm(args, torch, F, compeg_amd, images_of, resident, gpu, stream) if args.regions else
                antialias_arm(args, torch, compeg_amd, images_of, resident, gpu, stream))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        print(text, end="")
        return

    lines = [f"resized tensor output: {n} resident 4:2:2 DRI=4 frames per configuration, decoded once; {gpu.name()}",
             f"resized = Batch.pack_tensor_resized alone, HIP events on its stream; chain = pack_tensor(f32, k) -> F.interpolate(bilinear) -> "
             f"* scale + bias -> .to(dtype), per size group, launch by launch in turn; median of {args.reps} (min .. max)",
             f"{'configuration':<28} {'resized ms':>24} {'chain ms':>26} {'chain/resized':>13}"]
    slower = []
    for name, sizes, (ow, oh), dtype, k in CONFIGS:
        per = n // len(sizes)
        groups = [[images_of(w, h)[i % len(images_of(w, h))] for i in range(per)] for w, h in sizes]
        total = per * len(sizes)
        mixed = resident([im for g in groups for im in g])
        singles = [mixed] if len(sizes) == 1 else [resident(g) for g in groups]
        scale = [1.0] * 3 if dtype == "u8" else [1.0 / (255.0 * s) for s in STD]
        bias = [0.0] * 3 if dtype == "u8" else [-m / s for m, s in zip(MEAN, STD)]
        dst = torch.empty((total, 3, oh, ow), dtype=torch_type[dtype], device="cuda")
        ref = torch.empty((total, 3, oh, ow), dtype=torch_type[dtype], device="cuda")
        with torch.cuda.stream(stream):
            ts = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
            tb = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
            full = [torch.empty((per, 3, h // k, w // k), dtype=torch.float32, device="cuda") for w, h in sizes]

        def prime():
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < PRIME_SECONDS:
                mixed.decode(handle)
                mixed.wait()

        def resized():
            mixed.pack_tensor_resized(dst, (ow, oh), dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=handle)

        def chain():
            for g, (batch, tmp) in enumerate(zip(singles, full)):
                batch.pack_tensor(tmp, dtype="f32", downscale=k, hip_stream=handle)
                x = F.interpolate(tmp, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)
                x = x * ts + tb
                if dtype == "u8":
                    x = x.round().clamp(0, 255)
                ref[g * per:(g + 1) * per] = x.to(torch_type[dtype])

        with torch.cuda.stream(stream):
            for _ in range(2):   # warm-up of both: code objects, the allocator's blocks
                resized()
                chain()
            stream.synchronize()
            prime()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.reps)]
            for e0, e1, e2 in ev:
                e0.record(stream)
                resized()
                e1.record(stream)
                chain()
                e2.record(stream)
            stream.synchronize()
        t_new = [a.elapsed_time(b) for a, b, _ in ev]
        t_chain = [b.elapsed_time(c) for _, b, c in ev]
        mn, mc = statistics.median(t_new), statistics.median(t_chain)
        worst = float((dst.float() - ref.float()).abs().max())
        lines.append(f"{name:<28} {mn:8.3f} ({min(t_new):.3f} .. {max(t_new):.3f}) {mc:9.3f} ({min(t_chain):.3f} .. {max(t_chain):.3f}) "
                     f"{mc / mn:13.2f}   max |resized - chain| {worst:.4g}")
        spread = max(max(t_new) - min(t_new), max(t_chain) - min(t_chain))
        if mn - mc > spread:
            slower.append(name)
        del dst, ref, full, mixed, singles
        torch.cuda.empty_cache()

    lines.append("resized slower than the chain beside it by more than the rows' own min-to-max spread: " + ("; ".join(slower) if slower else "none"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
