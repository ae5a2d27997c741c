"""Developer tool (GPU box): what a colour map a sample costs in the resamplers' and the warp's stores.
  The workload: 4096 seeded crops (224 .. 448 pixels a side: the reductions below 2 that crop_scale leaves a resampler) of 16 pictures of
  1920 x 1080 random bytes, as views, a coin toss a crop for the mirror, to 224 x 224 float16 CHW RGB, top-down, under the ImageNet mean / std;
  one seeded ColorJitter matrix a crop (brightness, contrast, saturation 0.6 .. 1.4, hue -0.1 .. 0.1).  The tables are built once; a call is the C
  entry alone, timed by events on the stream around it.
  One configuration a process:
    unmapped  nhw_resample_to_tensor_device (warp: nhw_warp_to_tensor_device) -- with --lib, of another build of the library (the parent's);
    mapped    nhw_resample_mapped_to_tensor_device (nhw_warp_mapped_to_tensor_device) with the table of maps;
    torch     what a caller does without the maps: the unmapped call to float16 bytes (scale 1, bias 0), a per-sample 3 x 3 einsum plus offset,
              a clamp to 0 .. 255 and the normalisation, as torch passes;
    grey / grey_mapped  the one-channel calls on one-channel crops, a (gain, offset) pair a crop.
  `warm` calls, then `calls` timed ones: median / min / max in the JSON line it prints.  For the kernels' own times run one configuration with few
  calls under  rocprofv3 --kernel-trace --stats -- python tools/dev/gpu_colour_cost.py mapped cubic 3 1  (nothing else traced, started on its own).
usage: python tools/dev/gpu_colour_cost.py unmapped|mapped|torch|grey|grey_mapped two_tap|area|cubic|warp [calls=20] [warm=3] [--lib PATH]"""
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

CROPS, OUT, N_PICS, PIC_W, PIC_H = 4096, 224, 16, 1920, 1080
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main(config, kernel, calls, warm, lib_path):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    L = na._library()
    if lib_path:                                                     # another build: the unmapped entries alone, under this build's prototypes
        other = ctypes.CDLL(lib_path)
        for name in ("nhw_resample_to_tensor_device", "nhw_warp_to_tensor_device", "nhw_resample_grey_to_tensor_device", "nhw_warp_grey_to_tensor_device", "nhw_last_error"):
            getattr(other, name).argtypes, getattr(other, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
        L = other
    grey = config.startswith("grey")
    ch = 1 if grey else 3
    rng = np.random.default_rng(2400)
    pics = [torch.from_numpy(rng.integers(0, 256, (PIC_H, PIC_W, ch), dtype=np.uint8)).cuda() for _ in range(N_PICS)]
    table = np.zeros(CROPS, na.PICTURE_DTYPE)
    warps = np.zeros(CROPS, na.WARP_DTYPE)
    for i in range(CROPS):
        w, h = (int(v) for v in rng.integers(OUT, 2 * OUT + 1, 2))
        x, y, p = int(rng.integers(0, PIC_W - w + 1)), int(rng.integers(0, PIC_H - h + 1)), pics[i % N_PICS]
        table[i] = (p.data_ptr() + ch * (y * PIC_W + x), ch * PIC_W, w, h, 0, 0)
        a, b, c, d, e, f = na.warp_fixed(na.crop_warp(0, 0, w, h, (OUT, OUT), angle=math.radians(float(rng.uniform(-30, 30)))))
        warps[i] = (c, f, a, b, d, e, (0, 0, 0), 0, 0)
    flags = rng.integers(0, 2, CROPS).astype(np.uint8)
    jitter = [na.colour_matrix(*rng.uniform(0.6, 1.4, 3), hue=rng.uniform(-0.1, 0.1)) for _ in range(CROPS)]
    maps = na._colour_table([(float(m[0, 0]), float(m[0, 3])) for m in jitter] if grey else jitter, CROPS, "gpu_colour_cost", ch)
    if grey:
        fmt = na.TensorFormat(torch.float16, "CHW", "GREY", "reversed", mean=MEAN[0], std=STD[0])
    else:
        fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    raw = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0))
    out = torch.empty((CROPS, ch, OUT, OUT), dtype=torch.float16, device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
    d_tab, d_warps, d_maps, d_flags = dev(table), dev(warps), dev(maps), torch.from_numpy(flags).cuda()
    d_addr = (out.data_ptr() + torch.arange(CROPS, dtype=torch.int64) * (ch * OUT * OUT * 2)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    number = na.RESAMPLERS.get(kernel)
    M = torch.from_numpy(np.stack([m[:, :3] for m in jitter])).to("cuda", torch.float16)
    off = torch.from_numpy(np.stack([m[:, 3] for m in jitter])).to("cuda", torch.float16)[:, :, None, None]
    scale = torch.tensor(fmt.scale if not grey else [fmt.scale[0]], dtype=torch.float16, device="cuda")[None, :, None, None]
    bias = torch.tensor(fmt.bias if not grey else [fmt.bias[0]], dtype=torch.float16, device="cuda")[None, :, None, None]

    def call(f, mapped):
        c = f.c_struct()
        m = (d_maps.data_ptr(),) if mapped else ()
        if kernel == "warp":
            fn = L.nhw_warp_mapped_to_tensor_device if mapped else (L.nhw_warp_grey_to_tensor_device if grey else L.nhw_warp_to_tensor_device)
            rc = fn(d_tab.data_ptr(), CROPS, OUT, OUT, ctypes.byref(c), d_warps.data_ptr(), *m, d_addr.data_ptr(), stream)
        else:
            fn = L.nhw_resample_mapped_to_tensor_device if mapped else (L.nhw_resample_grey_to_tensor_device if grey else L.nhw_resample_to_tensor_device)
            rc = fn(d_tab.data_ptr(), CROPS, OUT, OUT, number, ctypes.byref(c), d_flags.data_ptr(), *m, d_addr.data_ptr(), stream)
        if rc:
            raise SystemExit(f"rc={rc}: {L.nhw_last_error().decode()}")

    def chain():
        call(raw, False)
        y = torch.einsum("nij,njhw->nihw", M, out) + off
        return y.clamp_(0, 255) * scale + bias

    run = {"unmapped": lambda: call(fmt, False), "grey": lambda: call(fmt, False), "mapped": lambda: call(fmt, True), "grey_mapped": lambda: call(fmt, True), "torch": chain}[config]
    ms = []
    for r in range(warm + calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run()
        t1.record()
        t1.synchronize()
        if r >= warm:
            ms.append(t0.elapsed_time(t1))
    ms.sort()
    print(json.dumps({"step": "colour", "config": config, "kernel": kernel, "lib": lib_path or "this", "crops": CROPS, "out": f"{OUT}x{OUT}", "calls": calls, "warm": warm,
                      "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    lib = None
    if "--lib" in a:
        lib = a[a.index("--lib") + 1]
        del a[a.index("--lib"):a.index("--lib") + 2]
    if len(a) < 2 or a[0] not in ("unmapped", "mapped", "torch", "grey", "grey_mapped") or a[1] not in ("two_tap", "area", "cubic", "warp"):
        sys.exit(__doc__)
    main(a[0], a[1], int(a[2]) if len(a) > 2 else 20, int(a[3]) if len(a) > 3 else 3, lib)
