"""Developer tool (GPU box): what the cubic filter costs, against the area kernel, the two-tap kernel and a plain copy.
  (a) section 19's case (a): 4096 seeded RandomResizedCrop rectangles of 16 pictures of 3840 x 2160 at q20 (gpu_crop_cost.py's draw), a coin
      toss a crop for the mirror, to 224 x 224 float16 CHW RGB top-down under the ImageNet mean / std; handles of max_batch 1024.
        Decoder.decode_crops_device(scale=None) with filter="cubic", "area" and "two_tap" in turn, the wall time of each call (all end
        synchronised); then k_cubic_to_tensor, k_area_to_tensor and k_resize_to_tensor alone over the same 4096 staged windows, in turn.
  (b) ingest, uint8 HWC: 4096 pictures of 500 x 375 to 224 x 224 (random bytes: no kernel looks at what it reads).  The three kernels alone.
  Every kernel figure: one warm-up launch, then hipEvents around each of `rounds` launches, median / min / max; GB/s is the source bytes read
  once plus the tensor written, over the median.  In the same run a device-to-device copy of as many bytes as the sources hold, timed the same way.
  A condition, not a measurement: in (a) the cubic call's first 64 crops equal resize_to_tensor_device(filter="cubic") of the staged windows.
Prints one JSON line.  One process, under a time limit of its own:
  timeout -k 10 900 python tools/dev/gpu_cubic_cost.py
usage: python tools/dev/gpu_cubic_cost.py [rounds=7]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from gpu_crop_cost import CROPS, MEAN, N_PICS, OUT, PIC_H, PIC_W, STD, _draw  # noqa: E402
from gpu_window_cost import _each, _pictures, _stat  # noqa: E402

FILTERS = ("cubic", "area", "two_tap")
KERNELS = {"cubic": "k_cubic_to_tensor", "area": "k_area_to_tensor", "two_tap": "k_resize_to_tensor"}


def _kernels(pictures, out_w, out_h, fmt, flips, rounds):
    """the three kernels alone over `pictures`, in turn, and a copy of as many bytes -> the figures"""
    import torch
    import nhwcodec_amd as na
    n = len(pictures)
    out = torch.empty((n,) + fmt.shape(out_h, out_w), dtype=fmt.dtype, device="cuda")
    table, _, _ = na._picture_table(pictures, "gpu_cubic_cost")
    addr = (out.data_ptr() + torch.arange(n, dtype=torch.int64) * (3 * out_h * out_w * out.element_size())).cuda()
    d_flags = torch.tensor(flips, dtype=torch.uint8, device="cuda") if flips is not None else None
    c = fmt.c_struct()
    lib, st = na._library(), torch.cuda.current_stream().cuda_stream
    rest = (ctypes.byref(c), d_flags.data_ptr() if d_flags is not None else None, addr.data_ptr(), st)
    src = sum(p.numel() for p in pictures)
    moved = src + out.numel() * out.element_size()
    a, b = torch.empty(src, dtype=torch.uint8, device="cuda"), torch.empty(src, dtype=torch.uint8, device="cuda")
    runs = [(KERNELS[f], (lambda v: lambda: lib.nhw_resample_to_tensor_device(table.data_ptr(), n, out_w, out_h, v, *rest))(na.RESAMPLERS[f])) for f in FILTERS]
    runs.append(("copy_of_the_source_bytes", lambda: b.copy_(a)))
    ms = {name: [] for name, _ in runs}
    for name, fn in runs * 2:                                       # in turn, twice: half the rounds each time
        ms[name] += _each(fn, (rounds + 1) // 2)
    res = {"source_bytes": src, "bytes_moved": moved, "source_pixels_per_output_pixel": round(src / 3 / (n * out_w * out_h), 2)}
    for name, v in ms.items():
        s = _stat(v)
        res[name] = {"ms": s, "GBps": round((2 * src if name.startswith("copy") else moved) / s["median"] / 1e6, 1)}
    res["cubic_over_area"] = round(res["k_cubic_to_tensor"]["ms"]["median"] / res["k_area_to_tensor"]["ms"]["median"], 2)
    return res


def main(rounds):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    res = {"step": "cubic", "rounds": rounds}
    # (a) the crops
    containers = _pictures(N_PICS, PIC_W, PIC_H, 20)
    rng = np.random.default_rng(2240)
    crops = _draw(rng, CROPS)
    flips = [bool(v) for v in rng.integers(0, 2, CROPS)]
    fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    dec = na.Decoder(0, max_batch=1024)
    batch = {f: torch.empty((CROPS, 3, OUT, OUT), dtype=torch.float16, device="cuda") for f in FILTERS}
    scales = []
    ms = {f: [] for f in batch}
    for r in range(rounds + 1):
        for f in batch:
            t0 = time.perf_counter()
            scales[:] = dec.decode_crops_device(containers, crops, (OUT, OUT), fmt, flips=flips, out=batch[f], filter=f)[1]
            if r:
                ms[f].append((time.perf_counter() - t0) * 1e3)
    diff = (batch["cubic"].float() - batch["area"].float()).abs()
    res["crops"] = {"crops": CROPS, "out": f"{OUT}x{OUT}", "picture": f"{N_PICS} of {PIC_W}x{PIC_H}", "scales": {s: scales.count(s) for s in (1, 2, 4)},
                    "call_wall_ms": {f: _stat(v) for f, v in ms.items()}, "cubic_against_area_mean_abs": round(float(diff.mean()), 5),
                    "cubic_against_area_max_abs": round(float(diff.max()), 4)}
    pictures, order = [], []
    for s in (1, 2, 4):
        idx = [i for i, v in enumerate(scales) if v == s]
        if idx:
            pictures += dec.decode_windows_device(containers, [(crops[i][0], *na.crop_window(*crops[i][1:], s)) for i in idx], s)
            order += idx
    dec.close()
    f_sorted = [flips[i] for i in order]
    alone = na.resize_to_tensor_device(pictures, (OUT, OUT), fmt, flips=f_sorted, filter="cubic")
    assert torch.equal(alone[[order.index(i) for i in range(64)]], batch["cubic"][:64])          # the condition
    del alone, batch
    res["crops"].update(_kernels(pictures, OUT, OUT, fmt, f_sorted, rounds))
    del pictures
    # (b) ingest
    u8 = na.TensorFormat("uint8", "HWC", "BGR", "file")
    gen = torch.Generator(device="cuda").manual_seed(20)
    src = torch.randint(0, 256, (4096, 375, 500, 3), dtype=torch.uint8, device="cuda", generator=gen)
    res["ingest_4096_of_500x375_to_224x224"] = _kernels(list(src), 224, 224, u8, None, rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and not a[0].isdigit():
        sys.exit(__doc__)
    main(int(a[0]) if a else 7)
