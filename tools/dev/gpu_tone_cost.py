"""Developer tool (GPU box): what a tone table a sample costs in the resamplers' and the warp's stores, and what the two histogram kernels
cost.
  The workload is gpu_colour_cost.py's: 4096 seeded crops (224 .. 448 pixels a side) of 16 pictures of 1920 x 1080 random bytes, as views, a coin
  toss a crop for the mirror, to 224 x 224 float16 CHW RGB, top-down, under the ImageNet mean / std; one seeded ColorJitter matrix and one seeded
  tone table (posterize, solarize, a gamma or their composition) a crop.  The tables are built once; a call is the C entry alone, timed by events
  on the stream around it.
  One configuration a process:
    unmapped  nhw_resample_to_tensor_device (warp: nhw_warp_to_tensor_device) -- with --lib, of another build of the library (the parent's);
    mapped    nhw_resample_mapped_to_tensor_device (nhw_warp_mapped_to_tensor_device) -- with --lib likewise;
    toned     nhw_resample_toned_to_tensor_device (nhw_warp_toned_to_tensor_device) with the maps and the tone tables;
    toned_only  the same with a null map table;
    torch     what a caller does without the tables: the mapped call to uint8 CHW RGB bytes, a per-sample gather through [n, 3, 256] tables and the
              normalisation, as torch passes;
    torch_equalize  the torch chain of Equalize behind the unmapped call to uint8: a bincount a sample and a channel, a cumulative sum, the
              table, a gather and the normalisation;
    grey / grey_mapped / grey_toned  the one-channel calls on one-channel crops;
    hist / hist_const / tone_from_hist / equalize  nhw_hist_device on a 4096 x 224 x 224 x 3 uint8 batch of random bytes, on a constant batch
              (every add on one bin: the worst case for the atomics), nhw_tone_from_hist_device on the random batch's histograms, and the
              whole device recipe (histograms, tables, the identity resample with the tables to float16); the kernel argument is ignored.
  `warm` calls, then `calls` timed ones: median / min / max in the JSON line it prints.
usage: python tools/dev/gpu_tone_cost.py CONFIG two_tap|area|cubic|warp [calls=20] [warm=3] [--lib PATH]"""
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

CROPS, OUT, N_PICS, PIC_W, PIC_H = 4096, 224, 16, 1920, 1080
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CONFIGS = ("unmapped", "mapped", "toned", "toned_only", "torch", "torch_equalize", "grey", "grey_mapped", "grey_toned", "hist", "hist_const", "tone_from_hist", "equalize")


def main(config, kernel, calls, warm, lib_path):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    L = na._library()
    if lib_path:                                                     # another build: the entries it has, under this build's prototypes
        other = ctypes.CDLL(lib_path)
        for name in ("nhw_resample_to_tensor_device", "nhw_warp_to_tensor_device", "nhw_resample_grey_to_tensor_device", "nhw_warp_grey_to_tensor_device",
                     "nhw_resample_mapped_to_tensor_device", "nhw_warp_mapped_to_tensor_device", "nhw_last_error"):
            getattr(other, name).argtypes, getattr(other, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
        L = other
    grey = config.startswith("grey")
    ch = 1 if grey else 3
    rng = np.random.default_rng(2400)
    stream = torch.cuda.current_stream().cuda_stream
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()

    if config in ("hist", "hist_const", "tone_from_hist", "equalize"):
        batch = torch.full((CROPS, OUT, OUT, 3), 131, dtype=torch.uint8, device="cuda") if config == "hist_const" else \
            torch.randint(0, 256, (CROPS, OUT, OUT, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(2500))
        table = np.zeros(CROPS, na.PICTURE_DTYPE)
        for i in range(CROPS):
            table[i] = (batch.data_ptr() + i * 3 * OUT * OUT, 3 * OUT, OUT, OUT, 0, 0)
        d_tab = dev(table)
        hist = torch.zeros((CROPS, 3, 256), dtype=torch.int32, device="cuda")
        tones = torch.zeros((CROPS, 768), dtype=torch.uint8, device="cuda")
        ops = torch.full((CROPS,), na.TONE_OPS["equalize"], dtype=torch.uint8, device="cuda")
        fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
        c = fmt.c_struct()
        out = torch.empty((CROPS, 3, OUT, OUT), dtype=torch.float16, device="cuda")
        d_addr = (out.data_ptr() + torch.arange(CROPS, dtype=torch.int64) * (3 * OUT * OUT * 2)).cuda()

        def check(rc):
            if rc:
                raise SystemExit(f"rc={rc}: {L.nhw_last_error().decode()}")
        do_hist = lambda: check(L.nhw_hist_device(d_tab.data_ptr(), CROPS, 3, hist.data_ptr(), stream))
        do_tone = lambda: check(L.nhw_tone_from_hist_device(hist.data_ptr(), CROPS, 3, ops.data_ptr(), tones.data_ptr(), stream))
        do_store = lambda: check(L.nhw_resample_toned_to_tensor_device(d_tab.data_ptr(), CROPS, OUT, OUT, 0, ctypes.byref(c), None, None, tones.data_ptr(), d_addr.data_ptr(), stream))
        do_hist()
        torch.cuda.synchronize()
        assert int(hist.sum()) == CROPS * 3 * OUT * OUT
        run = {"hist": do_hist, "hist_const": do_hist, "tone_from_hist": do_tone, "equalize": lambda: (do_hist(), do_tone(), do_store())}[config]
    else:
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
        maps = na._colour_table([(float(m[0, 0]), float(m[0, 3])) for m in jitter] if grey else jitter, CROPS, "gpu_tone_cost", ch)
        kinds = (lambda: na.tone_posterize(int(rng.integers(1, 8))), lambda: na.tone_solarize(int(rng.integers(0, 257))), lambda: na.tone_gamma(float(rng.uniform(0.5, 2.0))),
                 lambda: na.tone_compose(na.tone_gamma(float(rng.uniform(0.5, 2.0))), na.tone_posterize(int(rng.integers(2, 8)))))
        tabs = [kinds[int(rng.integers(0, 4))]() for _ in range(CROPS)]                 # uint8 [3, 256] on R, G, B
        tones = na._tone_arg([t[0] for t in tabs] if grey else tabs, CROPS, "gpu_tone_cost", ch)
        if grey:
            fmt = na.TensorFormat(torch.float16, "CHW", "GREY", "reversed", mean=MEAN[0], std=STD[0])
        else:
            fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
        raw = na.TensorFormat(torch.uint8, "CHW", "RGB", "reversed")
        out = torch.empty((CROPS, ch, OUT, OUT), dtype=torch.float16, device="cuda")
        out8 = torch.empty((CROPS, ch, OUT, OUT), dtype=torch.uint8, device="cuda")
        d_tab, d_warps, d_maps, d_flags, d_tones = dev(table), dev(warps), dev(maps), torch.from_numpy(flags).cuda(), torch.from_numpy(tones).cuda()
        d_addr = (out.data_ptr() + torch.arange(CROPS, dtype=torch.int64) * (ch * OUT * OUT * 2)).cuda()
        d_addr8 = (out8.data_ptr() + torch.arange(CROPS, dtype=torch.int64) * (ch * OUT * OUT)).cuda()
        number = na.RESAMPLERS.get(kernel)
        lut = torch.from_numpy(np.stack(tabs)).cuda()                                   # [n, 3, 256] on R, G, B, as out8's channels
        scale = torch.tensor(fmt.scale if not grey else [fmt.scale[0]], dtype=torch.float16, device="cuda")[None, :, None, None]
        bias = torch.tensor(fmt.bias if not grey else [fmt.bias[0]], dtype=torch.float16, device="cuda")[None, :, None, None]
        base = (torch.arange(CROPS * 3, device="cuda") * 256).view(CROPS, 3, 1)

        def call(f, mapped, toned=False, addr=d_addr, with_maps=True):
            c = f.c_struct()
            m = (d_maps.data_ptr() if with_maps else None, d_tones.data_ptr()) if toned else (d_maps.data_ptr(),) if mapped else ()
            if kernel == "warp":
                fn = L.nhw_warp_toned_to_tensor_device if toned else L.nhw_warp_mapped_to_tensor_device if mapped else (L.nhw_warp_grey_to_tensor_device if grey else L.nhw_warp_to_tensor_device)
                rc = fn(d_tab.data_ptr(), CROPS, OUT, OUT, ctypes.byref(c), d_warps.data_ptr(), *m, addr.data_ptr(), stream)
            else:
                fn = L.nhw_resample_toned_to_tensor_device if toned else L.nhw_resample_mapped_to_tensor_device if mapped else (
                    L.nhw_resample_grey_to_tensor_device if grey else L.nhw_resample_to_tensor_device)
                rc = fn(d_tab.data_ptr(), CROPS, OUT, OUT, number, ctypes.byref(c), d_flags.data_ptr(), *m, addr.data_ptr(), stream)
            if rc:
                raise SystemExit(f"rc={rc}: {L.nhw_last_error().decode()}")

        def chain():
            call(raw, True, addr=d_addr8)
            y = torch.gather(lut, 2, out8.view(CROPS, 3, -1).long()).view(CROPS, 3, OUT, OUT)
            return y.to(torch.float16) * scale + bias

        def chain_equalize():
            call(raw, False, addr=d_addr8)
            idx = out8.view(CROPS, 3, -1).long()
            h = torch.bincount((idx + base).view(-1), minlength=CROPS * 3 * 256).view(CROPS, 3, 256)
            total = h.sum(2, keepdim=True)
            last = torch.gather(h, 2, (255 - (h.flip(2) != 0).long().argmax(2, keepdim=True)))
            step = (total - last) // 255
            before = h.cumsum(2) - h
            t = torch.where(step > 0, ((before + step // 2) // step.clamp(min=1)).clamp(max=255), torch.arange(256, device="cuda").expand_as(h))
            t[:, :, 0] = 0
            y = torch.gather(t, 2, idx).view(CROPS, 3, OUT, OUT)
            return y.to(torch.float16) * scale + bias

        run = {"unmapped": lambda: call(fmt, False), "grey": lambda: call(fmt, False), "mapped": lambda: call(fmt, True), "grey_mapped": lambda: call(fmt, True),
               "toned": lambda: call(fmt, True, True), "grey_toned": lambda: call(fmt, True, True), "toned_only": lambda: call(fmt, False, True, with_maps=False),
               "torch": chain, "torch_equalize": chain_equalize}[config]
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
    print(json.dumps({"step": "tone", "config": config, "kernel": kernel, "lib": lib_path or "this", "crops": CROPS, "out": f"{OUT}x{OUT}", "calls": calls, "warm": warm,
                      "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    lib = None
    if "--lib" in a:
        lib = a[a.index("--lib") + 1]
        del a[a.index("--lib"):a.index("--lib") + 2]
    if len(a) < 2 or a[0] not in CONFIGS or a[1] not in ("two_tap", "area", "cubic", "warp"):
        sys.exit(__doc__)
    main(a[0], a[1], int(a[2]) if len(a) > 2 else 20, int(a[3]) if len(a) > 3 else 3, lib)
