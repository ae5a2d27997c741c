"""Developer tool (GPU box): what pictures of any size cost.
  (a) 4096 pictures of 500 x 375, packed (pitch 1500: rows not 16-byte aligned), one tile each;
  (b) 16 pictures of 3840 x 2160, packed (pitch 11 520, 16-byte aligned), 40 tiles each (640).
For each: k_tile_pad and k_untile_crop on their own (hipEvents around `repeats` launches), against a device-to-device copy of the same
tile bytes (torch copy_), then the host conveniences nhw_enc_pictures / nhw_dec_pictures against nhw_enc_batch / nhw_dec_batch on the same
tiles (handles of max_batch 1024, q20, wall time with the host copies).  Prints one JSON line per case.
usage: python tools/dev/gpu_picture_cost.py [case=a,b] [repeats=5]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

CASES = {"a": (4096, 500, 375, 1), "b": (16, 3840, 2160, 40)}      # pictures, W, H, tiles each


def _events(fn, repeats):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(repeats):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / repeats


def _wall(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def run(case, repeats):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    n, w, h, per = CASES[case]
    T = n * per
    pic_bytes = 3 * w * h
    # natural content: device-synthesised 512 x 512 images, laid out as pictures in one packed buffer
    enc = na.Encoder(0, max_batch=1024)
    synth = torch.cat([enc.synth_device(min(1024, T - i), i) for i in range(0, T, 1024)])
    packed = torch.empty(n * pic_bytes, dtype=torch.uint8, device="cuda")
    if per == 1:
        packed.as_strided((n, h, w, 3), (pic_bytes, 3 * w, 3, 1)).copy_(synth[:, :h, :w])
    else:
        ny, nx = -(-h // 512), -(-w // 512)
        big = synth.view(n, ny, nx, 512, 512, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, ny * 512, nx * 512, 3)
        packed.as_strided((n, h, w, 3), (pic_bytes, 3 * w, 3, 1)).copy_(big[:, :h, :w])
    views = [packed.as_strided((h, w, 3), (3 * w, 3, 1), i * pic_bytes) for i in range(n)]
    table, tiles_n, _ = na._picture_table(views, "cost")
    assert tiles_n == T
    tiles = torch.empty((T, 512, 512, 3), dtype=torch.uint8, device="cuda")
    L = na._library()
    st = torch.cuda.current_stream().cuda_stream
    t_pad = _events(lambda: L.nhw_tile_pictures_device(table.data_ptr(), n, 0, T, tiles.data_ptr(), st), repeats)
    out = torch.empty_like(packed)
    views_out = [out.as_strided((h, w, 3), (3 * w, 3, 1), i * pic_bytes) for i in range(n)]
    table_out, _, _ = na._picture_table(views_out, "cost")
    t_crop = _events(lambda: L.nhw_untile_pictures_device(tiles.data_ptr(), table_out.data_ptr(), n, 0, T, st), repeats)
    assert torch.equal(out, packed)
    src = torch.empty_like(tiles)
    t_copy = _events(lambda: tiles.copy_(src), repeats)
    # bytes each kernel must move: k_tile_pad reads the pictures and writes whole tiles; k_untile_crop reads from the tiles and writes
    # only the pictures' bytes; the copy reads and writes the tile bytes
    tile_bytes = T * na.IMG_BYTES
    pad_gbps, crop_gbps = (n * pic_bytes + tile_bytes) / t_pad / 1e6, 2 * n * pic_bytes / t_crop / 1e6
    copy_gbps = 2 * tile_bytes / t_copy / 1e6
    res = {"case": case, "pictures": n, "size": f"{w}x{h}", "tiles": T,
           "tile_pad_ms": round(t_pad, 4), "tile_pad_GBps": round(pad_gbps, 1),
           "untile_crop_ms": round(t_crop, 4), "untile_crop_GBps": round(crop_gbps, 1),
           "copy_ms": round(t_copy, 4), "copy_GBps": round(copy_gbps, 1),
           "tile_pad_vs_copy": round(pad_gbps / copy_gbps, 3), "untile_crop_vs_copy": round(crop_gbps / copy_gbps, 3)}
    # end to end: the host conveniences against the plain batch calls on the same tiles
    host_pics = packed.cpu().numpy()
    host_tiles = tiles.cpu().numpy()
    in_off = (np.arange(n + 1, dtype=np.uint64) * pic_bytes)
    wid, hei = np.full(n, w, np.uint32), np.full(n, h, np.uint32)
    arena = np.empty(16 * n + T * (4 + na.OUT_STRIDE), np.uint8)
    offs = np.empty(n + 1, np.uint64)
    status = np.empty(n, np.int32)
    rc = []
    res["enc_pictures_ms"] = round(_wall(lambda: rc.append(L.nhw_enc_pictures(enc.h, host_pics.ctypes.data, in_off.ctypes.data, wid.ctypes.data, hei.ctypes.data, n, 20,
                                                                             arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data)), repeats), 2)
    assert set(rc) == {0}, rc
    containers = na._split(arena, offs)
    b_arena = np.empty(1024 * na.OUT_STRIDE, np.uint8)
    b_offs = np.empty(1025, np.uint64)
    b_status = np.empty(1024, np.int32)
    files = []

    def plain_enc():
        files.clear()
        for i in range(0, T, 1024):
            m = min(1024, T - i)
            assert L.nhw_enc_batch(enc.h, host_tiles[i:].ctypes.data, m, 20, b_arena.ctypes.data, b_arena.size, b_offs.ctypes.data, b_status.ctypes.data) == 0
            files.extend(na._split(b_arena, b_offs[:m + 1]))
    res["enc_batch_ms"] = round(_wall(plain_enc, repeats), 2)
    enc.close()
    dec = na.Decoder(0, max_batch=1024)
    blob = np.frombuffer(b"".join(containers), np.uint8)
    c_off = np.zeros(n + 1, np.uint64)
    c_off[1:] = np.cumsum([len(c) for c in containers])
    px = np.empty(n * pic_bytes, np.uint8)
    res["dec_pictures_ms"] = round(_wall(lambda: rc.append(dec.lib.nhw_dec_pictures(dec.h, blob.ctypes.data, c_off.ctypes.data, n, px.ctypes.data, in_off.ctypes.data,
                                                                                    status.ctypes.data)), repeats), 2)
    assert set(rc) == {0} and not status.any(), status
    fblob = np.frombuffer(b"".join(files), np.uint8)
    f_off = np.zeros(T + 1, np.uint64)
    f_off[1:] = np.cumsum([len(f) for f in files])
    d_px = np.empty((1024, 512, 512, 3), np.uint8)
    d_st = np.empty(1024, np.int32)

    def plain_dec():
        for i in range(0, T, 1024):
            m = min(1024, T - i)
            assert dec.lib.nhw_dec_batch(dec.h, fblob.ctypes.data, f_off[i:].ctypes.data, m, d_px.ctypes.data, d_st.ctypes.data, None) == 0
    res["dec_batch_ms"] = round(_wall(plain_dec, repeats), 2)
    dec.close()
    print(json.dumps(res), flush=True)


def main(cases="a,b", repeats=5):
    import nhwcodec_amd as na
    na._library().nhw_dec_batch.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
    for c in cases.split(","):
        run(c, int(repeats))


if __name__ == "__main__":
    main(*sys.argv[1:])
