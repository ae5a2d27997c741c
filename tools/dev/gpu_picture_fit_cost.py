"""Developer tool (GPU box): what the picture searches cost.  Cases as in gpu_picture_cost.py (section 11):
  (a) 4096 pictures of 500 x 375, packed (pitch 1500: rows not 16-byte aligned), one tile each;
  (b) 16 pictures of 3840 x 2160, packed (pitch 11 520, 16-byte aligned), 40 tiles each (640).
For each: k_sse_crop on its own (hipEvents around `repeats` launches) over the case's tiles, against k_sse over the same tiles (both sides
whole tiles) and a device-to-device copy of the tile bytes in the same run.  Then (unless `kernels`) the two searches (handles of max_batch
1024, wall time with the host copies, best of `repeats`) against the stand-alone calls over the same (pictures, quality) pairs the walk
visited: nhw_enc_pictures of the pictures open at each rung, and for the PSNR search also nhw_dec_pictures of their containers plus
k_sse_crop over their tiles.  Prints one JSON line per case.
usage: python tools/dev/gpu_picture_fit_cost.py [case=a,b] [repeats=3] [kernels]"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

CASES = {"a": (4096, 500, 375, 1), "b": (16, 3840, 2160, 40)}      # pictures, W, H, tiles each
BYTE_LADDER = list(range(23, 16, -1))                                # 23 .. 17
PSNR_LADDER = list(range(17, 24))                                    # 17 .. 23


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


def _pictures(enc, case):
    """natural content: device-synthesised 512 x 512 images laid out as the case's pictures in one packed buffer"""
    import torch
    n, w, h, per = CASES[case]
    T = n * per
    pic_bytes = 3 * w * h
    synth = torch.cat([enc.synth_device(min(1024, T - i), i) for i in range(0, T, 1024)])
    packed = torch.empty(n * pic_bytes, dtype=torch.uint8, device="cuda")
    ny, nx = -(-h // 512), -(-w // 512)
    big = synth.view(n, ny, nx, 512, 512, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, ny * 512, nx * 512, 3)
    packed.as_strided((n, h, w, 3), (pic_bytes, 3 * w, 3, 1)).copy_(big[:, :h, :w])
    return packed, [packed.as_strided((h, w, 3), (3 * w, 3, 1), i * pic_bytes) for i in range(n)]


def run(case, repeats, kernels_only):
    import numpy as np
    import torch
    import nhwcodec_amd as na
    n, w, h, per = CASES[case]
    T = n * per
    pic_bytes = 3 * w * h
    enc = na.Encoder(0, max_batch=1024)
    packed, views = _pictures(enc, case)
    table, _, _ = na._picture_table(views, "cost")
    tiles = na.tile_pictures_device(views)
    other = torch.empty_like(tiles)
    other.copy_(tiles)
    L = na._library()
    st = torch.cuda.current_stream().cuda_stream
    sse = torch.zeros(n, dtype=torch.int64, device="cuda")
    sse_t = torch.zeros(T, dtype=torch.int64, device="cuda")
    t_crop = _events(lambda: L.nhw_sse_pictures_device(tiles.data_ptr(), table.data_ptr(), n, 0, T, sse.data_ptr(), st), repeats)
    t_sse = _events(lambda: L.nhw_sse_batch_device(tiles.data_ptr(), other.data_ptr(), T, sse_t.data_ptr(), st), repeats)
    t_copy = _events(lambda: other.copy_(tiles), repeats)
    # bytes each kernel must read: k_sse_crop the pictures' bytes from both sides, k_sse two whole tiles per tile; the copy reads and
    # writes the tile bytes
    tile_bytes = T * na.IMG_BYTES
    crop_gbps, sse_gbps, copy_gbps = 2 * n * pic_bytes / t_crop / 1e6, 2 * tile_bytes / t_sse / 1e6, 2 * tile_bytes / t_copy / 1e6
    res = {"case": case, "pictures": n, "size": f"{w}x{h}", "tiles": T,
           "sse_crop_ms": round(t_crop, 4), "sse_crop_GBps": round(crop_gbps, 1), "sse_crop_vs_copy": round(crop_gbps / copy_gbps, 3),
           "k_sse_ms": round(t_sse, 4), "k_sse_GBps": round(sse_gbps, 1), "copy_ms": round(t_copy, 4), "copy_GBps": round(copy_gbps, 1)}
    if kernels_only:
        print(json.dumps(res), flush=True)
        enc.close()
        return
    dec = na.Decoder(0, max_batch=1024)
    host = packed.cpu().numpy()
    pics = [host[i * pic_bytes:(i + 1) * pic_bytes].reshape(h, w, 3) for i in range(n)]
    # the targets: the median container size at q20 (bytes) and 36 dB (PSNR); every timing below is of the library call alone (the host
    # arrays are packed beforehand)
    budget = int(np.median([len(c) for c in _enc(enc, pics, 20)[0]]))
    P = lambda a: a.ctypes.data                                          # noqa: E731
    nn, blob, in_off, wid, hei, _, arena = enc._host_pictures(pics, "cost")
    offs, status, qual, sse_h = np.empty(nn + 1, np.uint64), np.empty(nn, np.int32), np.empty(nn, np.int32), np.empty(nn, np.uint64)
    lim = {"bytes": np.full(nn, budget, np.uint64), "psnr": np.full(nn, na.picture_psnr_to_max_sse(36.0, w, h), np.uint64)}
    lad = {"bytes": (ctypes.c_int * len(BYTE_LADDER))(*BYTE_LADDER), "psnr": (ctypes.c_int * len(PSNR_LADDER))(*PSNR_LADDER)}

    def fit(kind):
        if kind == "bytes":
            rc = L.nhw_enc_fit_pictures(enc.h, P(blob), P(in_off), P(wid), P(hei), nn, P(lim[kind]), lad[kind], len(lad[kind]), P(arena), arena.size,
                                        P(offs), P(status), P(qual))
        else:
            rc = L.nhw_enc_fit_sse_pictures(enc.h, dec.h, P(blob), P(in_off), P(wid), P(hei), nn, P(lim[kind]), lad[kind], len(lad[kind]), P(arena),
                                            arena.size, P(offs), P(status), P(qual), P(sse_h))
        assert rc == 0, rc
    for kind, ladder in (("bytes", BYTE_LADDER), ("psnr", PSNR_LADDER)):
        res[f"fit_{kind}_ms"] = round(_wall(lambda: fit(kind), repeats), 2)
        stats = enc.fit_stats()
        closes = [ladder.index(q) if s == 0 else len(ladder) for q, s in zip(qual.tolist(), status.tolist())]   # the rung each picture closed at
        rung_tiles, rung_ms = [], []
        for r in range(stats.rungs):
            open_ = [pics[i] for i in range(n) if closes[i] >= r]
            rung_tiles.append(len(open_) * per)
            conts, call = _enc(enc, open_, ladder[r])
            ms = _wall(call, 1)
            if kind == "psnr":
                ms += _wall(_dec_call(dec, conts), 1)
                sub = views[:len(open_)]                                     # the error pass over as many pictures of the case's shape
                tsub = tiles[:len(open_) * per]
                ssub = torch.zeros(len(sub), dtype=torch.int64, device="cuda")
                tb, _, _ = na._picture_table(sub, "cost")
                ms += _events(lambda: L.nhw_sse_pictures_device(tsub.data_ptr(), tb.data_ptr(), len(sub), 0, tsub.shape[0], ssub.data_ptr(), st), 1)
            rung_ms.append(ms)
        assert list(stats.images[:stats.rungs]) == rung_tiles, (kind, list(stats.images[:stats.rungs]), rung_tiles)
        res[f"{kind}_rungs"] = [list(stats.quality[:stats.rungs]), rung_tiles]
        res[f"{kind}_standalone_ms"] = round(sum(rung_ms), 2)
        res[f"{kind}_overhead_ms"] = round(res[f"fit_{kind}_ms"] - sum(rung_ms), 2)
        res[f"{kind}_status"] = {str(s): status.tolist().count(s) for s in sorted(set(status.tolist()))}
    res["byte_budget"] = budget
    enc.close()
    dec.close()
    print(json.dumps(res), flush=True)


def _enc(enc, pics, q):
    """nhw_enc_pictures of `pics` at q -> (the containers of the pictures whose tiles all encoded, the packed call for timing)"""
    import numpy as np
    n, blob, in_off, width, height, _, arena = enc._host_pictures(pics, "cost")
    offs = np.empty(n + 1, np.uint64)
    status = np.empty(n, np.int32)

    def call():
        enc._chk(enc.lib.nhw_enc_pictures(enc.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n, q,
                                          arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
    call()
    return [arena[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n) if status[i] == 0], call


def _dec_call(dec, containers):
    """the packed nhw_dec_pictures call of `containers`, for timing"""
    import numpy as np
    import nhwcodec_amd as na
    n = len(containers)
    shapes = [na.picture_info(c) for c in containers]
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in containers])
    blob = np.frombuffer(b"".join(containers), np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    out_off[1:] = np.cumsum([3 * w * h for w, h in shapes])
    out = np.empty(int(out_off[n]), np.uint8)
    status = np.empty(n, np.int32)

    def call():
        dec._chk(dec.lib.nhw_dec_pictures(dec.h, blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data, out_off.ctypes.data, status.ctypes.data))
        assert not status.any()
    return call


def main(cases="a,b", repeats=3, kernels=""):
    for c in cases.split(","):
        run(c, int(repeats), kernels == "kernels")


if __name__ == "__main__":
    main(*sys.argv[1:])
