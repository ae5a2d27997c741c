"""Developer tool (GPU box): what the affine warp costs, by angle and by walk, against the two-tap kernel.
  4096 entries of 256 x 256 random bytes -> 224 x 224 float16 CHW RGB top-down under the ImageNet mean / std, the output's centre on the
  source's, a step of 256 / 224 source pixels an output pixel, border colour 0.  For every angle of ANGLES (degrees): k_warp_to_tensor with
  every entry walked by rows, with every entry walked by 8 x 8 blocks (nhw_debug_warp_row_limit forces either) and as the kernel itself
  chooses; and k_resize_to_tensor on the same pictures and output size.  All arms interleaved in one process: three warm-up rounds, then
  hipEvents around each launch of `rounds` rounds, median / min, ms.  Prints one JSON line: {"two_tap": [median, min], "<angle>": {"d": the
  warp's d, "rows": [...], "blocks": [...], "rule": [...]}}.  One process, under a time limit of its own:
  timeout -k 10 300 python tools/dev/gpu_warp_cost.py
usage: python tools/dev/gpu_warp_cost.py [rounds=10]"""
import ctypes
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

N, SRC, OUT = 4096, 256, 224
ANGLES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 15, 30, 45, 90)
ROWS, BLOCKS, RULE = 1 << 22, -1, -2              # nhw_debug_warp_row_limit: rows for every entry; blocks for every entry; the rule's own limit


def main():
    import numpy as np
    import torch
    import nhwcodec_amd as na
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    L = na._library()
    fmt = na.TensorFormat("float16", "CHW", "RGB", "reversed", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    c = fmt.c_struct()
    src = torch.randint(0, 256, (N, SRC, SRC, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((N, 3, OUT, OUT), dtype=torch.float16, device="cuda")
    table = np.zeros(N, na.PICTURE_DTYPE)
    table["addr"] = src.data_ptr() + np.arange(N, dtype=np.uint64) * np.uint64(3 * SRC * SRC)
    table["pitch"], table["width"], table["height"] = 3 * SRC, SRC, SRC
    d_tab = torch.from_numpy(table.view(np.int64).copy()).cuda()
    addr = torch.from_numpy((np.uint64(out.data_ptr()) + np.arange(N, dtype=np.uint64) * np.uint64(3 * OUT * OUT * 2)).view(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def warps(deg):
        a, z = math.radians(deg), SRC / OUT
        lin = z * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        shift = np.array([SRC / 2, SRC / 2]) - lin @ np.array([OUT / 2, OUT / 2])
        six = na.warp_fixed(np.concatenate([lin, shift[:, None]], axis=1))
        w = np.zeros(N, na.WARP_DTYPE)
        for k, v in zip("abcdef", six):
            w[k] = v
        return torch.from_numpy(w.view(np.int64).copy()).cuda(), six[3]

    def warp(d_w, limit):
        L.nhw_debug_warp_row_limit(limit)
        try:
            return L.nhw_warp_to_tensor_device(d_tab.data_ptr(), N, OUT, OUT, ctypes.byref(c), d_w.data_ptr(), addr.data_ptr(), stream)
        finally:
            L.nhw_debug_warp_row_limit(RULE)

    arms = {("two_tap", ""): lambda: L.nhw_resample_to_tensor_device(d_tab.data_ptr(), N, OUT, OUT, 0, ctypes.byref(c), None, addr.data_ptr(), stream)}
    ds = {}
    for deg in ANGLES:
        d_w, ds[deg] = warps(deg)
        for name, limit in (("rows", ROWS), ("blocks", BLOCKS), ("rule", RULE)):
            arms[(deg, name)] = lambda d_w=d_w, limit=limit: warp(d_w, limit)
    times = {k: [] for k in arms}
    for rnd in range(3 + rounds):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = f()
            e1.record()
            torch.cuda.synchronize()
            if rc != 0:
                raise SystemExit(f"{k}: rc {rc}: {L.nhw_last_error().decode()}")
            if rnd >= 3:
                times[k].append(e0.elapsed_time(e1))
    stat = lambda v: [round(float(np.median(v)), 3), round(min(v), 3)]
    result = {"entries": N, "source": [SRC, SRC], "output": [OUT, OUT], "rounds": rounds, "two_tap": stat(times[("two_tap", "")])}
    for deg in ANGLES:
        result[str(deg)] = {"d": ds[deg], **{name: stat(times[(deg, name)]) for name in ("rows", "blocks", "rule")}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
