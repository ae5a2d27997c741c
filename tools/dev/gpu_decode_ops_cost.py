"""Developer tool (GPU box): what the per-sample flip, colour map and tone table cost in the full-file decode's last store.
  The batch of bench.py's decode leg -- `files` generator images (seeds 0 ..) encoded on the device at q20, the encoder's arena as the decoder's --
  decoded to float16 CHW RGB, top-down, under the ImageNet mean / std (grey: one channel, the first mean / std).  A coin toss a file for the mirror,
  one seeded ColorJitter matrix a file (brightness, contrast, saturation 0.6 .. 1.4, hue -0.1 .. 0.1; grey: its first gain and offset), one seeded
  gamma table a file (0.7 .. 1.4).  The tables are built once and stay referenced to the end; a call is the C entries alone, timed by events on the
  stream around it.
  The configurations, all in ONE process and taken in a seeded random order within every round, so that what shares the machine meets all of
  them alike and none always runs behind the same one:
    plain         nhw_dec_batch_device_tensor (grey: nhw_dec_batch_device_grey);
    plain_other   the same entry of another build of the library (--lib PATH: the parent's), on a handle of its own;
    flips, maps, tones, all   nhw_dec_batch_device_tensor_ops (_grey_ops) with that table alone, and with the three together;
    route         what a caller has without them: the uint8 decode (nhw_dec_batch_device_scaled; grey: nhw_dec_batch_device_grey without a format),
                  then nhw_resample_toned_to_tensor_device (two taps: the identity at the picture's own size S x S) with the same three tables.
  `warm` rounds that do not count, then `calls` rounds: median / min / max a configuration in the JSON line it prints; the spread of plain and
  plain_other is the run-to-run noise a difference has to clear.
usage: python tools/dev/gpu_decode_ops_cost.py colour|grey 1|2|4 [calls=20] [warm=3] [files=4096] [--lib PATH]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main(kind, scale, calls, warm, n, lib_path):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    grey = kind == "grey"
    ch, side = (1 if grey else 3), 512 // scale
    enc = na.Encoder(0, n, device_only=True)
    files, sizes, status = enc.encode_device(enc.synth_device(n, 0), 20)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    enc.close()
    dec = na.Decoder(0, n)
    L = dec.lib
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * na.OUT_STRIDE
    rng = np.random.default_rng(2800)
    flags = rng.integers(0, 2, n).astype(np.uint8)
    jitter = [na.colour_matrix(*rng.uniform(0.6, 1.4, 3), hue=rng.uniform(-0.1, 0.1)) for _ in range(n)]
    gammas = [na.tone_gamma(float(g)) for g in rng.uniform(0.7, 1.4, n)]
    maps = na._colour_table([(float(m[0, 0]), float(m[0, 3])) for m in jitter] if grey else jitter, n, "gpu_decode_ops_cost", ch)
    tabs = na._tone_arg([g[0] for g in gammas] if grey else gammas, n, "gpu_decode_ops_cost", ch)
    if grey:
        fmt = na.TensorFormat(torch.float16, "CHW", "GREY", "reversed", mean=MEAN[0], std=STD[0])
    else:
        fmt = na.TensorFormat(torch.float16, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    c = fmt.c_struct()
    out = torch.empty((n, ch, side, side), dtype=torch.float16, device="cuda")
    px = torch.empty((n, side, side, ch), dtype=torch.uint8, device="cuda")
    st, qq = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    d_flags, d_maps, d_tones = torch.from_numpy(flags).cuda(), na._device_table(maps, torch.device("cuda", 0)), torch.from_numpy(tabs).cuda()
    table = np.zeros(n, na.PICTURE_DTYPE)                           # the decoded slots as pictures of S x S
    for i in range(n):
        table[i] = (px.data_ptr() + i * ch * side * side, ch * side, side, side, 0, 0)
    d_table = torch.from_numpy(table.view(np.int64).copy()).cuda()
    d_addr = (out.data_ptr() + torch.arange(n, dtype=torch.int64) * (ch * side * side * 2)).cuda()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    head = (files.data_ptr(), offs.data_ptr(), sizes.data_ptr(), n, scale)
    tail = (st.data_ptr(), qq.data_ptr(), s)

    def chk(rc, lib=L):
        if rc:
            raise SystemExit(f"rc={rc}: {(lib.nhw_dec_last_error() or lib.nhw_last_error()).decode()}")

    def plain(lib, h):
        chk((lib.nhw_dec_batch_device_grey if grey else lib.nhw_dec_batch_device_tensor)(h, *head, ctypes.byref(c), out.data_ptr(), *tail), lib)

    def ops(f, m, t):
        chk((L.nhw_dec_batch_device_grey_ops if grey else L.nhw_dec_batch_device_tensor_ops)(dec.h, *head, ctypes.byref(c), f, m, t, out.data_ptr(), *tail))

    def route():
        if grey:
            chk(L.nhw_dec_batch_device_grey(dec.h, *head, None, px.data_ptr(), *tail))
        else:
            chk(L.nhw_dec_batch_device_scaled(dec.h, *head, px.data_ptr(), *tail))
        chk(L.nhw_resample_toned_to_tensor_device(d_table.data_ptr(), n, side, side, na.RESAMPLERS["two_tap"], ctypes.byref(c), d_flags.data_ptr(), d_maps.data_ptr(),
                                                  d_tones.data_ptr(), d_addr.data_ptr(), s))

    F, M, T = d_flags.data_ptr(), d_maps.data_ptr(), d_tones.data_ptr()
    run = {"plain": lambda: plain(L, dec.h), "flips": lambda: ops(F, None, None), "maps": lambda: ops(None, M, None), "tones": lambda: ops(None, None, T),
           "all": lambda: ops(F, M, T), "route": route}
    other_h = None
    if lib_path:                                                     # another build: its plain entry on its own handle, under this build's prototypes
        other = ctypes.CDLL(lib_path)
        for name in ("nhw_dec_create", "nhw_dec_destroy", "nhw_dec_batch_device_tensor", "nhw_dec_batch_device_grey", "nhw_dec_last_error", "nhw_last_error"):
            getattr(other, name).argtypes, getattr(other, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
        other_h = ctypes.c_void_p()
        chk(other.nhw_dec_create(0, n, ctypes.byref(other_h)), other)
        run["plain_other"] = lambda: plain(other, other_h)
    ms = {k: [] for k in run}
    names = list(run)
    with torch.cuda.stream(stream):
        for r in range(warm + calls):
            for k in rng.permutation(names):                         # a seeded order a round: no configuration always follows the same one
                f = run[str(k)]
                k = str(k)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if r >= warm:
                    ms[k].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    line = {"step": "decode_ops", "kind": kind, "scale": scale, "files": n, "quality": 20, "dtype": "float16", "calls": calls, "warm": warm, "lib": lib_path or None}
    for k, v in ms.items():
        v.sort()
        line[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    print(json.dumps(line), flush=True)
    if other_h is not None:
        other.nhw_dec_destroy(other_h)
    dec.close()
    del d_flags, d_maps, d_tones, d_table, d_addr, out, px                # (referenced up to here: the calls above hold their addresses)


if __name__ == "__main__":
    a = sys.argv[1:]
    lib = None
    if "--lib" in a:
        lib = a[a.index("--lib") + 1]
        del a[a.index("--lib"):a.index("--lib") + 2]
    if len(a) < 2 or a[0] not in ("colour", "grey") or a[1] not in ("1", "2", "4"):
        sys.exit(__doc__)
    main(a[0], int(a[1]), int(a[2]) if len(a) > 2 else 20, int(a[3]) if len(a) > 3 else 3, int(a[4]) if len(a) > 4 else 4096, lib)
