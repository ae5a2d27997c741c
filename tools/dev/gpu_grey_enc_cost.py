"""Developer tool (GPU box): what a grey encode costs against the colour encode of the same pictures replicated into B = G = R.
  The workload: `n` grey pictures (default 4096), the green channel of Encoder.synth_device's batch made contiguous, at each quality of `qualities`
  (default 23, 20, 17, 10: the plain front kernel, the fused one in two families, the low path); one handle of max_batch n.
  In one process, in turn, Encoder.encode_grey_device and Encoder.encode_device on the replicated pictures into the same output tensors: `warm`
  warm-up rounds and `rounds` timed ones (10 or more for a figure that is written down).  A round's time is taken twice: by a pair of events around the call, and from the handle's own
  nhw_enc_last_timing (total_ms, front_ms) read after the synchronise that ends the round.  The replication pass (one pointwise copy, 1 byte a pixel
  read and 3 written) is timed by events on its own.  Every run is printed, with the median and the spread (max - min) of each list.
  Every tensor whose address the library has been given -- the pictures, the replicated pictures, the outputs -- is held in `keep` until after the
  last synchronise (section 26 records what a script that freed one early cost).
Prints one JSON line a quality.  One process, under a time limit of its own; for the kernels' own times run it with few rounds under
  rocprofv3 --kernel-trace --stats -- python tools/dev/gpu_grey_enc_cost.py 2 1 256
usage: python tools/dev/gpu_grey_enc_cost.py [rounds=10] [warm=2] [n=4096] [qualities=23,20,17,10]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def _stats(v):
    s = sorted(v)
    return {"runs": [round(x, 3) for x in v], "median": round(s[len(s) // 2], 3), "spread": round(s[-1] - s[0], 3)}


def main(rounds, warm, n, qualities):
    import torch
    import nhwcodec_amd as na
    enc = na.Encoder(0, max_batch=n, device_only=True)
    keep = []
    bgr = enc.synth_device(n, seed_base=4000)
    grey = bgr[:, :, :, 1].contiguous()
    out = enc.alloc_out(n)
    keep += [bgr, grey, out]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rep_ms = []
    rep = torch.empty((n, 512, 512, 3), dtype=torch.uint8, device="cuda")
    for r in range(warm + rounds):
        a, b = ev(), ev()
        a.record()
        rep.copy_(grey.unsqueeze(3).expand(n, 512, 512, 3))
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            rep_ms.append(a.elapsed_time(b))
    keep.append(rep)
    assert bool((rep[:, :, :, 0] == grey).all()) and bool((rep[:, :, :, 2] == grey).all())
    for q in qualities:
        ms = {k: [] for k in ("grey_event", "grey_total", "grey_front", "colour_event", "colour_total", "colour_front")}
        same = None
        for r in range(warm + rounds):
            files = {}
            for name, call, src in (("colour", enc.encode_device, rep), ("grey", enc.encode_grey_device, grey)):
                a, b = ev(), ev()
                a.record()
                o, sizes, status = call(src, q, out=out)
                b.record()
                torch.cuda.synchronize()
                t = enc.timing()
                if r >= warm:
                    ms[name + "_event"].append(a.elapsed_time(b)); ms[name + "_total"].append(t.total_ms); ms[name + "_front"].append(t.front_ms)
                if r == 0:
                    files[name] = (sizes.clone(), status.clone(), o[:, :4096].clone())
            if r == 0:                                                 # the two calls wrote the same files (their first 4096 bytes, sizes and status)
                same = all(bool((x == y).all()) for x, y in zip(files["grey"], files["colour"]))
        res = {"step": "grey_enc", "q": q, "n": n, "rounds": rounds, "warm": warm, "same_files": same, "replicate_ms": _stats(rep_ms)}
        res.update({k: _stats(v) for k, v in ms.items()})
        for k in ("event", "total", "front"):
            res[f"grey_over_colour_{k}"] = round(res[f"grey_{k}"]["median"] / res[f"colour_{k}"]["median"], 3)
        print(json.dumps(res), flush=True)
    torch.cuda.synchronize()
    enc.close()
    del keep


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and not a[0].isdigit():
        sys.exit(__doc__)
    main(int(a[0]) if a else 10, int(a[1]) if len(a) > 1 else 2, int(a[2]) if len(a) > 2 else 4096,
         [int(x) for x in a[3].split(",")] if len(a) > 3 else [23, 20, 17, 10])
