"""Developer tool (GPU box): what windows cost, against the paths that were there before them.
  crops: section 13's case -- 4096 crops of 224 x 224 at seeded positions out of 16 pictures of 3840 x 2160 at q20, handles of max_batch
      1024 -- by nhw_dec_windows_to_device at scale 1, by nhw_dec_regions_to_device and by nhw_dec_pictures followed by slices on the
      host: the three calls in turn, `repeats` rounds after a warm-up round, the wall time of each call (it ends in its synchronise), with
      the tiles decoded and the bytes uploaded.  A condition, not a measurement: the window call decodes at most 640 tiles and writes what
      the region call writes.  Then k_untile_window alone over the call's use table (hipEvents around each launch; bytes read plus written
      over the best launch) next to a device-to-device copy of the same bytes in the same run; the decode time of the window call's last
      chunk comes from nhw_dec_last_timing.
  viewport: one 1024 x 768 window of one 16384 x 16384 picture (q20) at scales 2 and 4 by nhw_dec_windows, against nhw_dec_pictures_scaled
      of the whole picture and against nhw_dec_regions of the covering full-scale rectangle; the same rounds and statistics.
Prints one JSON line per step.  One step a process, each under a time limit of its own, the next only if the one before succeeded:
  timeout -k 10 400 python tools/dev/gpu_window_cost.py crops && timeout -k 10 500 python tools/dev/gpu_window_cost.py viewport
usage: python tools/dev/gpu_window_cost.py crops|viewport [repeats=5]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

N_PICS, PIC_W, PIC_H, PER = 16, 3840, 2160, 40                     # section 13's case (b)
CROP, CROPS = 224, 4096
BIG_SIDE, VIEW_W, VIEW_H = 16384, 1024, 768


def _stat(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def _rounds(calls, repeats):
    """the calls in turn, one warm-up round and `repeats` timed ones -> the wall times (ms) of every call, by name"""
    ms = {name: [] for name, _ in calls}
    for r in range(repeats + 1):
        for name, fn in calls:
            t0 = time.perf_counter()
            fn()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: _stat(v) for name, v in ms.items()}


def _each(fn, repeats):
    """the time of each of `repeats` launches of fn (ms), after one that is not counted"""
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(repeats + 1)]
    ev[0].record()
    for i in range(repeats):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(repeats)]


def _pictures(n, w, h, quality):
    """n generated pictures of w x h (tiles of the device generator side by side, cropped) -> their containers"""
    import numpy as np
    import nhwcodec_amd as na
    ny, nx = -(-h // 512), -(-w // 512)
    enc = na.Encoder(0, max_batch=1024)
    out = []
    for i in range(n):                                              # picture after picture: the host never holds more than one of them twice
        synth = enc.synth_device(ny * nx, i * ny * nx)
        pic = synth.view(ny, nx, 512, 512, 3).permute(0, 2, 1, 3, 4).reshape(ny * 512, nx * 512, 3)[:h, :w].contiguous().cpu().numpy()
        del synth
        out += enc.encode_pictures([pic], quality)
    enc.close()
    return out


def _blob(containers):
    import numpy as np
    off = np.zeros(len(containers) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    return np.frombuffer(b"".join(containers), np.uint8), off


def crops(repeats):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    n, w, h, per = N_PICS, PIC_W, PIC_H, PER
    ny, nx = -(-h // 512), -(-w // 512)
    containers = _pictures(n, w, h, 20)
    rng = np.random.default_rng(224)
    rects = [(i % n, int(rng.integers(0, w - CROP + 1)), int(rng.integers(0, h - CROP + 1)), CROP, CROP) for i in range(CROPS)]
    dec = na.Decoder(0, max_batch=1024)
    L, H = dec.lib, dec.h
    blob, off = _blob(containers)
    table = np.array(rects, np.uint32)                              # nhw_rect: five 32-bit fields
    batches = {k: torch.zeros((CROPS, CROP, CROP, 3), dtype=torch.uint8, device="cuda") for k in ("windows", "regions")}
    addr = {k: np.array([b[i].data_ptr() for i in range(CROPS)], np.uint64) for k, b in batches.items()}
    pitch = np.full(CROPS, 3 * CROP, np.uint64)
    status = np.empty(CROPS, np.int32)
    host = np.empty((CROPS, CROP, CROP, 3), np.uint8)
    px = np.empty(n * 3 * w * h, np.uint8)
    px_off = np.arange(n, dtype=np.uint64) * np.uint64(3 * w * h)
    pst = np.empty(n, np.int32)
    rc, stats = [], {}

    def windows():
        rc.append(L.nhw_dec_windows_to_device(H, blob.ctypes.data, off.ctypes.data, n, table.ctypes.data, CROPS, 1, addr["windows"].ctypes.data,
                                              pitch.ctypes.data, status.ctypes.data))
        rc.append(int(np.abs(status).sum()))

    def regions():
        rc.append(L.nhw_dec_regions_to_device(H, blob.ctypes.data, off.ctypes.data, n, table.ctypes.data, CROPS, addr["regions"].ctypes.data,
                                              pitch.ctypes.data, status.ctypes.data))
        rc.append(int(np.abs(status).sum()))

    def whole():
        rc.append(L.nhw_dec_pictures(H, blob.ctypes.data, off.ctypes.data, n, px.ctypes.data, px_off.ctypes.data, pst.ctypes.data))
        rc.append(int(np.abs(pst).sum()))
        p = px.reshape(n, h, w, 3)
        for i, (ci, x, y, _, _) in enumerate(rects):
            host[i] = p[ci, y:y + CROP, x:x + CROP]

    res = {"step": "crops", "crops": CROPS, "size": f"{CROP}x{CROP}", "pictures": n, "picture": f"{w}x{h}", "repeats": repeats}
    res["wall_ms"] = _rounds([("dec_windows_to_device", windows), ("dec_regions_to_device", regions), ("dec_pictures_and_slices", whole)], repeats)
    assert set(rc) == {0}
    windows()
    stats["windows"] = dec.region_stats()
    last = dec.timing()
    regions()
    stats["regions"] = dec.region_stats()
    torch.cuda.synchronize()
    assert stats["windows"][0] <= n * per, stats                    # the condition: at most the 640 tiles there are ...
    assert torch.equal(batches["windows"], batches["regions"])      # ... and the region call's outputs
    assert np.array_equal(batches["windows"].cpu().numpy(), host)
    res["windows_tiles_decoded"], res["windows_bytes_uploaded"] = stats["windows"]
    res["regions_tiles_decoded"], res["regions_bytes_uploaded"] = stats["regions"]
    res["pictures_tiles_decoded"], res["pictures_bytes_uploaded"] = n * per, sum(len(c) for c in containers)
    res["windows_last_chunk_decode_ms"] = round(last.total_ms, 3)
    # the kernel alone: all 640 decoded tiles as the slots, one use per (crop, tile)
    p = px.reshape(n, h, w, 3)
    padded = np.stack([np.pad(q, ((0, 512 * ny - h), (0, 512 * nx - w), (0, 0)), mode="edge") for q in p])
    tiles = torch.from_numpy(np.ascontiguousarray(padded.reshape(n, ny, 512, nx, 512, 3).transpose(0, 1, 3, 2, 4, 5)).reshape(n * per, 512, 512, 3)).cuda()
    regs = np.zeros(CROPS, na.REGION_DTYPE)
    uses = []
    out = torch.zeros_like(batches["windows"])
    for i, (ci, x, y, _, _) in enumerate(rects):
        regs[i] = (out[i].data_ptr(), 3 * CROP, x, y, CROP, CROP, w, h, 0, 0)
        uses += [(i, ci * per + ty * nx + tx, tx, ty) for ty in range(y // 512, (y + CROP - 1) // 512 + 1) for tx in range(x // 512, (x + CROP - 1) // 512 + 1)]
    uses.sort(key=lambda u: u[1])
    d_regs = torch.from_numpy(regs.view(np.uint8).copy()).cuda()
    d_uses = torch.from_numpy(np.array(uses, np.uint32).view(np.uint8).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    lib = na._library()
    t_k = _each(lambda: lib.nhw_untile_windows_device(tiles.data_ptr(), d_regs.data_ptr(), CROPS, d_uses.data_ptr(), len(uses), 0, n * per, 1, st), repeats)
    assert torch.equal(out, batches["windows"])
    src = torch.empty_like(out)
    t_c = _each(lambda: src.copy_(out), repeats)
    moved = 2 * out.numel()                                         # bytes read plus bytes written, for both
    res.update({"uses": len(uses), "untile_window_ms": _stat(t_k), "untile_window_GBps": round(moved / min(t_k) / 1e6, 1),
                "copy_ms": _stat(t_c), "copy_GBps": round(moved / min(t_c) / 1e6, 1)})
    dec.close()
    print(json.dumps(res), flush=True)


def viewport(repeats):
    import numpy as np
    import nhwcodec_amd as na
    side = BIG_SIDE
    containers = _pictures(1, side, side, 20)
    blob, off = _blob(containers)
    dec = na.Decoder(0, max_batch=1024)
    L, H = dec.lib, dec.h
    res = {"step": "viewport", "picture": f"{side}x{side}", "window": f"{VIEW_W}x{VIEW_H}", "repeats": repeats,
           "picture_tiles": na.picture_tiles(side, side), "container_bytes": len(containers[0])}
    for scale in (2, 4):
        ss = side // scale
        x, y = (3 * ss) // 8 + 17, (5 * ss) // 16 + 5                # off the tile grid
        rect = np.array([(0, x, y, VIEW_W, VIEW_H)], np.uint32)
        cover = np.array([(0, x * scale, y * scale, VIEW_W * scale, VIEW_H * scale)], np.uint32)
        win = np.empty(3 * VIEW_W * VIEW_H, np.uint8)
        reg = np.empty(3 * VIEW_W * VIEW_H * scale * scale, np.uint8)
        whole = np.empty(3 * ss * ss, np.uint8)
        zero, st = np.zeros(1, np.uint64), np.empty(1, np.int32)
        rc, stats = [], {}

        def windows():
            rc.append(L.nhw_dec_windows(H, blob.ctypes.data, off.ctypes.data, 1, rect.ctypes.data, 1, scale, win.ctypes.data, zero.ctypes.data, st.ctypes.data))
            rc.append(int(st[0]))

        def scaled():
            rc.append(L.nhw_dec_pictures_scaled(H, blob.ctypes.data, off.ctypes.data, 1, scale, whole.ctypes.data, zero.ctypes.data, st.ctypes.data))
            rc.append(int(st[0]))

        def regions():
            rc.append(L.nhw_dec_regions(H, blob.ctypes.data, off.ctypes.data, 1, cover.ctypes.data, 1, reg.ctypes.data, zero.ctypes.data, st.ctypes.data))
            rc.append(int(st[0]))

        r = {"at": f"{x},{y}", "wall_ms": _rounds([("dec_windows", windows), ("dec_pictures_scaled", scaled), ("dec_regions_covering", regions)], repeats)}
        assert set(rc) == {0}
        windows()
        r["windows_tiles_decoded"], r["windows_bytes_uploaded"] = dec.region_stats()
        regions()
        r["regions_tiles_decoded"], r["regions_bytes_uploaded"] = dec.region_stats()
        assert np.array_equal(win.reshape(VIEW_H, VIEW_W, 3), whole.reshape(ss, ss, 3)[y:y + VIEW_H, x:x + VIEW_W])
        res[f"scale_{scale}"] = r
    dec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] in ("crops", "viewport"):
        {"crops": crops, "viewport": viewport}[a[0]](int(a[1]) if len(a) > 1 else 5)
    else:
        sys.exit(__doc__)
