"""Developer tool (GPU box): what the distortion search costs beyond its encodes, decodes and error passes.  n device-synthesised images,
every image's target the median SSE at quality `mid` (the median PSNR there).  For each ladder (lo..23 for every lo given) it prints the
fit call's time and per-rung image counts, the sum of stand-alone encode + decode + SSE times at the same (images, quality) pairs, and the
difference (gather + select + compaction + the wait per rung).  It also times the SSE kernel alone on n image pairs.
usage: python tools/dev/gpu_fit_psnr_cost.py [n=4096] [mid=18] [repeats=3] [lo=1,17]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main(n=4096, mid=18, repeats=3, los=(1, 17)):
    import torch
    import nhwcodec_amd as na
    enc = na.Encoder(0, max_batch=n, device_only=True)
    dec = na.Decoder(0, max_batch=n)
    bgr = enc.synth_device(n, 0)
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * na.OUT_STRIDE
    o, s, st = enc.encode_device(bgr, mid)
    px, dst, _ = dec.decode_device(o, offs, s)
    sse = na.sse_device(bgr, px)
    torch.cuda.synchronize()
    good = (st == 0) & (dst == 0)
    target = int(sse[good].double().median().item())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        fn()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    sse_ms = min(timed(lambda: na.sse_device(bgr, px)) for _ in range(repeats))
    res = {"images": n, "target_quality": mid, "target_sse": target, "target_psnr_db": round(10 * __import__("math").log10(na.PEAK_SSE_NUMERATOR / target), 3),
           "sse_kernel_ms": round(sse_ms, 4), "sse_kernel_tb_s": round(2 * n * na.IMG_BYTES / sse_ms / 1e9, 3), "ladders": []}
    out = enc.alloc_out(n) + (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"))
    plain = enc.alloc_out(n)
    for lo in los:
        ladder = list(range(lo, 24))
        enc.encode_fit_psnr_device(bgr, dec, max_sse=target, ladder=ladder, out=out)     # warm-up: the first call allocates the search's buffers
        torch.cuda.synchronize()
        fits = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            enc.encode_fit_psnr_device(bgr, dec, max_sse=target, ladder=ladder, out=out)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            fs = enc.fit_stats()
            fits.append((fs.total_ms, wall))
        pairs = [(fs.quality[r], fs.images[r]) for r in range(fs.rungs)]
        # stand-alone encode + decode + SSE of as many images at the same qualities (the first m images: the same count, not the same images)
        sums = []
        for _ in range(repeats):
            tot = 0.0
            for q, m in pairs:
                def step():
                    oo, ss, _ = enc.encode_device(bgr[:m], q, out=plain)
                    pp, _, _ = dec.decode_device(oo, offs[:m], ss[:m], out=px)
                    na.sse_device(bgr[:m], pp[:m])
                tot += timed(step)
            sums.append(tot)
        fit_ms = min(f[0] for f in fits)
        res["ladders"].append({"ladder": f"{lo}..23", "rungs": [{"q": q, "images": m} for q, m in pairs],
                               "fit_ms": [round(f[0], 3) for f in fits], "fit_host_wall_ms": [round(f[1], 3) for f in fits],
                               "standalone_sum_ms": [round(x, 3) for x in sums], "overhead_ms": round(fit_ms - min(sums), 3),
                               "gather_images": sum(m for _, m in pairs[1:])})
    print(json.dumps(res))
    dec.close()
    enc.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    kw = {}
    if len(a) > 0: kw["n"] = int(a[0])
    if len(a) > 1: kw["mid"] = int(a[1])
    if len(a) > 2: kw["repeats"] = int(a[2])
    if len(a) > 3: kw["los"] = tuple(int(x) for x in a[3].split(","))
    main(**kw)
