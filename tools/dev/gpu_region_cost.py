"""Developer tool (GPU box): what a rectangle of a picture costs.
  kernel a | kernel b: k_untile_region on whole-picture regions of gpu_picture_cost.py's cases -- (a) 4096 pictures of 500 x 375, packed
      (pitch 1500: rows not 16-byte aligned), one tile each; (b) 16 pictures of 3840 x 2160, packed, 40 tiles each -- against k_untile_crop
      on the same tiles and against a device-to-device copy of the tile bytes, all in one run: hipEvents around each of `repeats`
      launches, so that the spread of the launches is seen next to the gap between the kernels.
  crops: 4096 crops of 224 x 224 at seeded positions out of the 16 pictures of case (b), encoded at q20: the kernel alone into an
      [4096, 224, 224, 3] batch tensor (time, GB/s over the bytes stored), then nhw_dec_regions_to_device into that tensor against
      nhw_dec_pictures of the 16 containers followed by slicing on the host (wall time, best of `repeats`, handles of max_batch 1024), with
      the tiles decoded and the bytes uploaded of each.
Prints one JSON line per step.  One step a process, each under a time limit of its own, the next only if the one before succeeded:
  timeout -k 10 300 python tools/dev/gpu_region_cost.py kernel a && timeout -k 10 300 python tools/dev/gpu_region_cost.py kernel b &&
  timeout -k 10 400 python tools/dev/gpu_region_cost.py crops
usage: python tools/dev/gpu_region_cost.py kernel a|b [repeats=5]  |  crops [repeats=5]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

CASES = {"a": (4096, 500, 375, 1), "b": (16, 3840, 2160, 40)}      # pictures, W, H, tiles each
CROP, CROPS = 224, 4096


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


def _stat(ms):
    s = sorted(ms)
    return {"min": round(s[0], 4), "median": round(s[len(s) // 2], 4), "max": round(s[-1], 4)}


def _region_table(rows):
    """rows of (addr, pitch, x, y, w, h, W, H) -> the nhw_region table as a CUDA tensor, first_tile running"""
    import numpy as np
    import torch
    import nhwcodec_amd as na
    table = np.zeros(len(rows), na.REGION_DTYPE)
    first = 0
    for i, r in enumerate(rows):
        table[i] = (*r, first, 0)
        first += na.region_tiles(r[6], r[7], *r[2:6])
    return torch.from_numpy(table.view(np.uint8).copy()).cuda(), first


def kernel(case, repeats):
    import torch
    import nhwcodec_amd as na
    n, w, h, per = CASES[case]
    T, pic_bytes = n * per, 3 * w * h
    tiles = torch.randint(0, 256, (T, 512, 512, 3), dtype=torch.uint8, device="cuda")
    L = na._library()
    st = torch.cuda.current_stream().cuda_stream
    outs = [torch.full((n * pic_bytes,), 7, dtype=torch.uint8, device="cuda") for _ in range(2)]
    views = [outs[0].as_strided((h, w, 3), (3 * w, 3, 1), i * pic_bytes) for i in range(n)]
    table, tiles_n, _ = na._picture_table(views, "cost")
    regs, first = _region_table([(outs[1].data_ptr() + i * pic_bytes, 3 * w, 0, 0, w, h, w, h) for i in range(n)])
    assert tiles_n == first == T
    t_crop = _each(lambda: L.nhw_untile_pictures_device(tiles.data_ptr(), table.data_ptr(), n, 0, T, st), repeats)
    t_reg = _each(lambda: L.nhw_untile_regions_device(tiles.data_ptr(), regs.data_ptr(), n, 0, T, st), repeats)
    assert torch.equal(outs[0], outs[1])
    src = torch.empty_like(tiles)
    t_copy = _each(lambda: tiles.copy_(src), repeats)
    gbps = lambda ms, b: round(b / min(ms) / 1e6, 1)                # best launch
    crop_g, reg_g, copy_g = gbps(t_crop, 2 * n * pic_bytes), gbps(t_reg, 2 * n * pic_bytes), gbps(t_copy, 2 * T * na.IMG_BYTES)
    print(json.dumps({"step": "kernel", "case": case, "pictures": n, "size": f"{w}x{h}", "tiles": T,
                      "untile_crop_ms": _stat(t_crop), "untile_region_ms": _stat(t_reg), "copy_ms": _stat(t_copy),
                      "untile_crop_GBps": crop_g, "untile_region_GBps": reg_g, "copy_GBps": copy_g,
                      "untile_crop_vs_copy": round(crop_g / copy_g, 3), "untile_region_vs_copy": round(reg_g / copy_g, 3),
                      "region_vs_crop_time": round(min(t_reg) / min(t_crop), 3)}), flush=True)


def _wall(fn, repeats):
    fn()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def crops(repeats):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    n, w, h, per = CASES["b"]
    T = n * per
    enc = na.Encoder(0, max_batch=1024)
    synth = enc.synth_device(T, 0)
    ny, nx = -(-h // 512), -(-w // 512)
    big = synth.view(n, ny, nx, 512, 512, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, ny * 512, nx * 512, 3)[:, :h, :w].cpu().numpy()
    containers = enc.encode_pictures([np.ascontiguousarray(p) for p in big], 20)
    enc.close()
    del synth
    rng = np.random.default_rng(224)
    rects = [(i % n, int(rng.integers(0, w - CROP + 1)), int(rng.integers(0, h - CROP + 1)), CROP, CROP) for i in range(CROPS)]
    dec = na.Decoder(0, max_batch=1024)
    batch = torch.zeros((CROPS, CROP, CROP, 3), dtype=torch.uint8, device="cuda")
    # the kernel alone: the decoded tiles of every selection, gathered in running order
    pics = dec.decode_pictures(containers)
    order = []
    for ci, x, y, rw, rh in rects:
        order += [ci * per + ty * nx + tx for ty in range(y // 512, (y + rh - 1) // 512 + 1) for tx in range(x // 512, (x + rw - 1) // 512 + 1)]
    padded = np.stack([np.pad(p, ((0, 512 * ny - h), (0, 512 * nx - w), (0, 0)), mode="edge") for p in pics])
    all_tiles = torch.from_numpy(np.ascontiguousarray(padded.reshape(n, ny, 512, nx, 512, 3).transpose(0, 1, 3, 2, 4, 5)).reshape(T, 512, 512, 3)).cuda()
    sel = all_tiles[torch.tensor(order, device="cuda")].contiguous()
    regs, first = _region_table([(batch[i].data_ptr(), 3 * CROP, x, y, CROP, CROP, w, h) for i, (_, x, y, _, _) in enumerate(rects)])
    assert first == len(order)
    L = na._library()
    st = torch.cuda.current_stream().cuda_stream
    t_k = _each(lambda: L.nhw_untile_regions_device(sel.data_ptr(), regs.data_ptr(), CROPS, 0, first, st), repeats)
    want = np.stack([pics[ci][y:y + CROP, x:x + CROP] for ci, x, y, _, _ in rects])
    assert np.array_equal(batch.cpu().numpy(), want)
    stored = CROPS * CROP * CROP * 3
    res = {"step": "crops", "crops": CROPS, "size": f"{CROP}x{CROP}", "pictures": n, "selected_tiles": first,
           "untile_region_ms": _stat(t_k), "untile_region_GBps_stored": round(stored / min(t_k) / 1e6, 1)}
    del sel, all_tiles
    # end to end: the regions into the batch tensor against whole pictures and slices on the host
    batch.zero_()
    torch.cuda.synchronize()
    blob = np.frombuffer(b"".join(containers), np.uint8)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in containers])
    table = np.array(rects, np.uint32)                              # nhw_rect: five 32-bit fields
    addr = np.array([batch[i].data_ptr() for i in range(CROPS)], np.uint64)
    pitch = np.full(CROPS, 3 * CROP, np.uint64)
    status = np.empty(CROPS, np.int32)
    rc = []
    res["dec_regions_to_device_ms"] = round(_wall(lambda: rc.append(dec.lib.nhw_dec_regions_to_device(
        dec.h, blob.ctypes.data, off.ctypes.data, n, table.ctypes.data, CROPS, addr.ctypes.data, pitch.ctypes.data, status.ctypes.data)), repeats), 2)
    assert set(rc) == {0} and not status.any()
    res["regions_tiles_decoded"], res["regions_bytes_uploaded"] = dec.region_stats()
    assert np.array_equal(batch.cpu().numpy(), want)
    host = np.empty_like(want)
    px = np.empty(n * 3 * w * h, np.uint8)
    px_off = np.arange(n, dtype=np.uint64) * np.uint64(3 * w * h)
    pst = np.empty(n, np.int32)

    def whole():
        rc.append(dec.lib.nhw_dec_pictures(dec.h, blob.ctypes.data, off.ctypes.data, n, px.ctypes.data, px_off.ctypes.data, pst.ctypes.data))
        p = px.reshape(n, h, w, 3)
        for i, (ci, x, y, _, _) in enumerate(rects):
            host[i] = p[ci, y:y + CROP, x:x + CROP]
    res["dec_pictures_and_slices_ms"] = round(_wall(whole, repeats), 2)
    assert set(rc) == {0} and not pst.any() and np.array_equal(host, want)
    res["pictures_tiles_decoded"], res["pictures_bytes_uploaded"] = T, sum(len(c) for c in containers)
    dec.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "kernel" and len(a) >= 2 and a[1] in CASES:
        kernel(a[1], int(a[2]) if len(a) > 2 else 5)
    elif a and a[0] == "crops":
        crops(int(a[1]) if len(a) > 1 else 5)
    else:
        sys.exit(__doc__)
