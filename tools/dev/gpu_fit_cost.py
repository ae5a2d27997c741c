"""Developer tool (GPU box): what the byte-budget search costs beyond its encodes.  n device-synthesised images, the ladder top..1, every
image's budget the median size at the top quality.  Prints the fit call's time and per-rung image counts, the sum of stand-alone
nhw_enc_batch_device times at the same (images, quality) pairs, and the difference (gather + select + compaction + the wait per rung).
usage: python tools/dev/gpu_fit_cost.py [n=4096] [top=20] [repeats=3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main(n=4096, top=20, repeats=3):
    import torch
    import nhwcodec_amd as na
    enc = na.Encoder(0, max_batch=n, device_only=True)
    bgr = enc.synth_device(n, 0)
    _, s_top, st_top = enc.encode_device(bgr, top)
    torch.cuda.synchronize()
    budget = int(s_top[st_top == 0].float().median().item())
    ladder = list(range(top, 0, -1))
    out = enc.alloc_out(n) + (torch.empty(n, dtype=torch.int32, device="cuda"),)
    enc.encode_fit_device(bgr, budget, ladder, out=out)               # warm-up: the first fit call allocates the search's buffers
    torch.cuda.synchronize()
    fits = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        enc.encode_fit_device(bgr, budget, ladder, out=out)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        st = enc.fit_stats()
        fits.append((st.total_ms, wall))
    pairs = [(st.quality[r], st.images[r]) for r in range(st.rungs)]
    # stand-alone encodes of as many images at the same qualities (the first m images: the same count, not the same images)
    plain = enc.alloc_out(n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    sums = []
    for _ in range(repeats):
        tot = 0.0
        for q, m in pairs:
            enc.encode_device(bgr[:m], q, out=plain)
            ev[0].record()
            enc.encode_device(bgr[:m], q, out=plain)
            ev[1].record()
            torch.cuda.synchronize()
            tot += ev[0].elapsed_time(ev[1])
        sums.append(tot)
    fit_ms = min(f[0] for f in fits)
    enc_ms = min(sums)
    print(json.dumps({"images": n, "ladder_top": top, "budget_bytes": budget, "rungs": [{"q": q, "images": m} for q, m in pairs],
                      "fit_ms": [round(f[0], 3) for f in fits], "fit_host_wall_ms": [round(f[1], 3) for f in fits],
                      "standalone_encode_sum_ms": [round(s, 3) for s in sums], "overhead_ms": round(fit_ms - enc_ms, 3),
                      "gather_images": sum(m for _, m in pairs[1:])}))
    enc.close()


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*a)
