"""Developer tool (GPU box): what crops resized into one batch tensor cost, against what there was before them.
  The workload is section 15's case (a) with RandomResizedCrop's rectangles: 4096 seeded crops out of 16 pictures of 3840 x 2160 at q20,
  areas 8 % .. 100 % of the picture, aspects 3/4 .. 4/3 (both uniform; a rectangle that does not fit is drawn again), a coin toss a crop
  for the mirror, to 224 x 224 float16 CHW RGB top-down under the ImageNet mean / std; handles of max_batch 1024.
    crops:  Decoder.decode_crops_device(scale=None) -- every crop at crop_scale, one C call a scale.
    before: Decoder.decode_windows_device at scale 1, `chunk` crops a call (the windows of all 4096 crops are some 50 GB), then per crop
            torch.nn.functional.interpolate(mode="bilinear", antialias=False) of the permuted float window, the mirror, the normalisation
            and the cast into the slot of the batch tensor.  Not the same numbers: torch interpolates in float and from the full scale.
  The two in turn, one warm-up round and 7 timed ones, the wall time of each (both end synchronised); then the tiles decoded and the
  tile-file bytes uploaded of each scale group (region_stats), and k_resize_to_tensor alone over all 4096 staged windows (hipEvents
  around each launch; bytes read plus written over the best launch).  A condition, not a measurement: the first 64 crops equal
  resize_to_tensor_device of decode_windows_device's windows.
Prints one JSON line.  One process, under a time limit of its own:
  timeout -k 10 900 python tools/dev/gpu_crop_cost.py
usage: python tools/dev/gpu_crop_cost.py [rounds=7] [chunk=256]"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from gpu_window_cost import _each, _pictures, _stat  # noqa: E402

N_PICS, PIC_W, PIC_H = 16, 3840, 2160
CROPS, OUT = 4096, 224
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _draw(rng, n):
    """n crops (picture, x, y, w, h): area 8 % .. 100 % of the picture, aspect w / h in 3/4 .. 4/3"""
    out = []
    while len(out) < n:
        area = rng.uniform(0.08, 1.0) * PIC_W * PIC_H
        aspect = rng.uniform(3 / 4, 4 / 3)
        w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 1 <= w <= PIC_W and 1 <= h <= PIC_H:
            out.append((len(out) % N_PICS, int(rng.integers(0, PIC_W - w + 1)), int(rng.integers(0, PIC_H - h + 1)), w, h))
    return out


def main(rounds, chunk):
    import numpy as np
    import torch
    import torch.nn.functional as F
    import nhwcodec_amd as na
    containers = _pictures(N_PICS, PIC_W, PIC_H, 20)
    rng = np.random.default_rng(2240)
    crops = _draw(rng, CROPS)
    flips = [bool(v) for v in rng.integers(0, 2, CROPS)]
    fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    dec = na.Decoder(0, max_batch=1024)
    batch = torch.empty((CROPS, 3, OUT, OUT), dtype=torch.float16, device="cuda")
    old = torch.empty_like(batch)
    sc = torch.tensor(fmt.scale, device="cuda").view(3, 1, 1)
    bi = torch.tensor(fmt.bias, device="cuda").view(3, 1, 1)
    scales = []

    def new():
        scales[:] = dec.decode_crops_device(containers, crops, (OUT, OUT), fmt, flips=flips, out=batch)[1]

    def before():
        for c0 in range(0, CROPS, chunk):
            wins = dec.decode_windows_device(containers, crops[c0:c0 + chunk], 1)
            for i, win in enumerate(wins, c0):
                x = win.flip(0).permute(2, 0, 1).flip(0).unsqueeze(0).float()      # top-down, RGB, [1, 3, h, w]
                y = F.interpolate(x, size=(OUT, OUT), mode="bilinear", antialias=False)[0]
                if flips[i]:
                    y = y.flip(2)
                old[i] = y * sc + bi
        torch.cuda.synchronize()

    ms = {"decode_crops_device": [], "windows_then_interpolate": []}
    for r in range(rounds + 1):
        for name, fn in (("decode_crops_device", new), ("windows_then_interpolate", before)):
            t0 = time.perf_counter()
            fn()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    res = {"step": "crops", "crops": CROPS, "out": f"{OUT}x{OUT}", "pictures": N_PICS, "picture": f"{PIC_W}x{PIC_H}", "rounds": rounds, "chunk": chunk,
           "wall_ms": {k: _stat(v) for k, v in ms.items()}, "scales": {s: scales.count(s) for s in (1, 2, 4)}}
    diff = (batch.float() - old.float()).abs()
    res["against_torch_max_abs"], res["against_torch_mean_abs"] = round(float(diff.max()), 4), round(float(diff.mean()), 5)
    # each scale group on its own: its tiles and bytes, and its staged windows for the kernel alone
    pictures, order, groups = [], [], {}
    for s in (1, 2, 4):
        idx = [i for i, v in enumerate(scales) if v == s]
        if not idx:
            continue
        rects = [(crops[i][0], *na.crop_window(*crops[i][1:], s)) for i in idx]
        t0 = time.perf_counter()
        dec.decode_crops_device(containers, rects, (OUT, OUT), fmt, flips=[flips[i] for i in idx], scale=s)
        wall = (time.perf_counter() - t0) * 1e3
        tiles, nbytes = dec.region_stats()
        groups[s] = {"crops": len(idx), "tiles_decoded": tiles, "bytes_uploaded": nbytes, "window_pixels": sum(r[3] * r[4] for r in rects), "wall_ms": round(wall, 3)}
        pictures += dec.decode_windows_device(containers, rects, s)
        order += idx
    res["groups"] = groups
    res["tiles_there_are"] = N_PICS * na.picture_tiles(PIC_W, PIC_H)
    f_sorted = [flips[i] for i in order]
    alone = na.resize_to_tensor_device(pictures, (OUT, OUT), fmt, flips=f_sorted)
    first = [order.index(i) for i in range(64)]
    assert torch.equal(alone[first], batch[:64])                        # the condition
    table, _, dev = na._picture_table(pictures, "gpu_crop_cost")
    addr = (alone.data_ptr() + torch.arange(CROPS, dtype=torch.int64) * (3 * OUT * OUT * 2)).cuda()
    d_flags = torch.tensor(f_sorted, dtype=torch.uint8, device="cuda")
    c = fmt.c_struct()
    import ctypes
    lib, st = na._library(), torch.cuda.current_stream().cuda_stream
    t_k = _each(lambda: lib.nhw_resize_to_tensor_device(table.data_ptr(), CROPS, OUT, OUT, ctypes.byref(c), d_flags.data_ptr(), addr.data_ptr(), st), rounds)
    moved = sum(p.numel() for p in pictures) + alone.numel() * 2        # the windows' bytes read once, the tensor written
    res.update({"resize_kernel_ms": _stat(t_k), "resize_kernel_GBps": round(moved / min(t_k) / 1e6, 1), "resize_kernel_bytes": moved})
    dec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and not a[0].isdigit():
        sys.exit(__doc__)
    main(int(a[0]) if a else 7, int(a[1]) if len(a) > 1 else 256)
