"""Developer tool (GPU box): what the grey crops, warps and windows cost against the colour calls on the same inputs.
  The workload is section 18's (gpu_crop_cost.py's draw): 4096 seeded RandomResizedCrop rectangles of 16 pictures of 3840 x 2160 at q20, a coin
  toss a crop for the mirror, to 224 x 224 float16, top-down, under the ImageNet mean / std (the grey format takes the first channel's); handles
  of max_batch 1024.
    crops:   Decoder.decode_crops_device against decode_crops_grey_device, scale=None, for each of the three filters;
    warps:   Decoder.decode_warps_device against decode_warps_grey_device, scale=None, the same rectangles turned by 0 and by 30 degrees;
    windows: Decoder.decode_windows_device against decode_windows_grey_device at scale 1, into preallocated tensors, the first `windows` crops
             (the windows of all 4096 are some 50 GB).
  The two of a pair in turn, `warm` warm-up rounds and `rounds` timed ones, the wall time of every call (each ends synchronised) -- every run is
  printed.  The bytes a pixel the resampler moves are computed from the shapes: the staged windows' bytes read once plus the tensor written.
Prints one JSON line.  One process, under a time limit of its own; for the kernels' own times run it with few rounds under
  rocprofv3 --kernel-trace --stats -- python tools/dev/gpu_grey_cost.py 2 1
usage: python tools/dev/gpu_grey_cost.py [rounds=6] [warm=2] [windows=128]"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from gpu_crop_cost import CROPS, MEAN, N_PICS, OUT, PIC_H, PIC_W, STD, _draw  # noqa: E402
from gpu_window_cost import _pictures  # noqa: E402


def _pair(colour, grey, rounds, warm):
    ms = {"colour": [], "grey": []}
    for r in range(warm + rounds):
        for name, fn in (("colour", colour), ("grey", grey)):
            t0 = time.perf_counter()
            fn()
            if r >= warm:
                ms[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    ms["grey_over_colour_median"] = round(sorted(ms["grey"])[len(ms["grey"]) // 2] / sorted(ms["colour"])[len(ms["colour"]) // 2], 3)
    return ms


def main(rounds, warm, n_windows):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    containers = _pictures(N_PICS, PIC_W, PIC_H, 20)
    rng = np.random.default_rng(2240)
    crops = _draw(rng, CROPS)
    flips = [bool(v) for v in rng.integers(0, 2, CROPS)]
    colour = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    grey = na.TensorFormat(torch.float16, "CHW", "GREY", "reversed", mean=MEAN[0], std=STD[0])
    dec = na.Decoder(0, max_batch=1024)
    batch3 = torch.empty((CROPS, 3, OUT, OUT), dtype=torch.float16, device="cuda")
    batch1 = torch.empty((CROPS, 1, OUT, OUT), dtype=torch.float16, device="cuda")
    res = {"step": "grey", "crops": CROPS, "out": f"{OUT}x{OUT}", "pictures": N_PICS, "picture": f"{PIC_W}x{PIC_H}", "rounds": rounds, "warm": warm, "wall_ms": {}}
    scales = []

    def sync(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run

    for f in ("two_tap", "area", "cubic"):
        res["wall_ms"][f"crops_{f}"] = _pair(sync(lambda: scales.__setitem__(slice(None), dec.decode_crops_device(containers, crops, (OUT, OUT), colour, flips=flips, out=batch3, filter=f)[1])),
                                             sync(lambda: dec.decode_crops_grey_device(containers, crops, (OUT, OUT), grey, flips=flips, out=batch1, filter=f)), rounds, warm)
    res["scales"] = {s: scales.count(s) for s in (1, 2, 4)}
    # the staged windows' pixels: what the resampler reads, once, at 3 or 1 bytes a pixel; it writes 3 or 1 float16 an output pixel
    window_px = sum(w * h for _, _, w, h in (na.crop_window(*c[1:], s) for c, s in zip(crops, scales)))
    out_px = CROPS * OUT * OUT
    res["resampler_bytes_a_output_pixel"] = {"colour": round((3 * window_px + 6 * out_px) / out_px, 2), "grey": round((window_px + 2 * out_px) / out_px, 2)}
    which = [c[0] for c in crops]
    for deg in (0, 30):
        mats = [na.crop_warp(x, y, w, h, (OUT, OUT), angle=math.radians(deg), flip=fl) for (_, x, y, w, h), fl in zip(crops, flips)]
        res["wall_ms"][f"warps_{deg}_degrees"] = _pair(sync(lambda: dec.decode_warps_device(containers, which, mats, (OUT, OUT), colour, out=batch3)),
                                                       sync(lambda: dec.decode_warps_grey_device(containers, which, mats, (OUT, OUT), grey, out=batch1)), rounds, warm)
    del batch3, batch1
    rects = crops[:n_windows]
    out3 = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for _, _, _, w, h in rects]
    out1 = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _, _, _, w, h in rects]
    res["wall_ms"][f"windows_scale_1_first_{n_windows}"] = _pair(sync(lambda: dec.decode_windows_device(containers, rects, 1, out=out3)),
                                                                 sync(lambda: dec.decode_windows_grey_device(containers, rects, 1, out=out1)), rounds, warm)
    res["windows_tiles_decoded"] = dec.region_stats()[0]
    dec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and not a[0].isdigit():
        sys.exit(__doc__)
    main(int(a[0]) if a else 6, int(a[1]) if len(a) > 1 else 2, int(a[2]) if len(a) > 2 else 128)
