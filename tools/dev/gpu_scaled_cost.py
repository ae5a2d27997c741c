"""Developer tool (GPU box): what a decode at scale 1, 2 and 4 costs.
The batch of bench.py's decode leg -- 4096 generator images (seeds 0 ..) encoded on the device at q20, the encoder's arena as the decoder's --
decoded on ONE handle at the given scale: `warmup` calls that do not count, then `repeats` calls, Decoder.timing() read after each.  Prints one
JSON line: the median, the smallest and the largest total_ms (their spread is the run-to-run noise a comparison has to clear), the medians of
entropy_ms and recon_ms (recon_ms: k_dec_final at scale 1, k_dec_scaled<S> else), and for scales 2 and 4 the algorithmic bytes of
k_dec_scaled<S> a file (the luma plane as stored + the two chroma planes as stored + the picture) with the bandwidth recon_ms makes of them.
One scale a process; under rocprofv3 --kernel-trace --stats the program goes behind `--`, and `repeats` can be small:
  timeout -k 10 300 python tools/dev/gpu_scaled_cost.py 1 && timeout -k 10 300 python tools/dev/gpu_scaled_cost.py 2 && timeout -k 10 300 python tools/dev/gpu_scaled_cost.py 4
usage: python tools/dev/gpu_scaled_cost.py 1|2|4 [repeats=20] [warmup=3] [files=4096]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

# k_dec_scaled<S> reads, a file: S = 2: 256 x 256 int16 of plane_l1 + 2 x 65536 chroma bytes; S = 4: 128 x 128 int16 of plane A + 2 x 128 x 128 int16
ALGORITHMIC_BYTES = {2: 131072 + 2 * 65536 + 196608, 4: 32768 + 2 * 32768 + 49152}


def main():
    import torch
    import nhwcodec_amd as na
    scale = int(sys.argv[1])
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
    enc = na.Encoder(0, n, device_only=True)
    files, sizes, status = enc.encode_device(enc.synth_device(n, 0), 20)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    dec = na.Decoder(0, n)
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * na.OUT_STRIDE
    side = 512 // scale
    out = torch.empty((n, side, side, 3), dtype=torch.uint8, device="cuda")
    rows = []
    for i in range(warmup + repeats):
        _, st, _ = dec.decode_scaled_device(files, offs, sizes, scale, out)
        torch.cuda.synchronize()
        t = dec.timing()
        if i >= warmup:
            rows.append((t.total_ms, t.entropy_ms, t.recon_ms))
    assert int(st.abs().sum()) == 0
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    line = {"scale": scale, "files": n, "quality": 20, "repeats": repeats, "warmup": warmup,
            "total_ms": {"median": round(med(0), 4), "min": round(min(r[0] for r in rows), 4), "max": round(max(r[0] for r in rows), 4)},
            "entropy_ms": round(med(1), 4), "recon_ms": round(med(2), 4)}
    if scale in ALGORITHMIC_BYTES:
        line["k_dec_scaled_bytes_per_file"] = ALGORITHMIC_BYTES[scale]
        line["k_dec_scaled_GBps_by_recon_ms"] = round(n * ALGORITHMIC_BYTES[scale] / (med(2) * 1e-3) / 1e9, 1)
    print(json.dumps(line))
    dec.close()
    enc.close()


if __name__ == "__main__":
    main()
