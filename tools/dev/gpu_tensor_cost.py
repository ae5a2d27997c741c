"""Developer tool (GPU box): what a decode into a training tensor costs.
The batch of bench.py's decode leg -- 4096 generator images (seeds 0 ..) encoded on the device at q20, the encoder's arena as the decoder's --
decoded on ONE handle, on one torch stream: `warmup` calls that do not count, then `repeats` calls, each between two events of that stream.
  bytes   decode_scaled_device: the byte path (it runs on a checkout without tensor formats too: the parent against this commit)
  fused   decode_tensor_device at DTYPE / CHW / RGB / reversed with the ImageNet mean and std
  chain   the same tensor without the fused store: decode_scaled_device, then torch's flip (rows and channels), permute + cast (one copy_ into
          the [n, 3, S, S] result) and the affine (mul_, add_ with [1, 3, 1, 1] constants), all on the same stream
Prints one JSON line: the median, the smallest and the largest ms of the whole call (their spread is the run-to-run noise a comparison has to
clear), the medians of the decoder's own total_ms and recon_ms (Decoder.timing(): the last kernel), and for that last kernel the algorithmic
bytes a file -- what it reads (scale 1: the 2.05 GB a 4096-file batch of section 7.2's PMC figure; scales 2, 4: the planes of section 14) plus
the 3 S S elements it writes -- with the TB/s recon_ms makes of them, to be held against the device-copy rates of section 13's table.
One configuration a process; under rocprofv3 --kernel-trace --stats the program goes behind `--`, and `repeats` can be small.
usage: python tools/dev/gpu_tensor_cost.py bytes|fused|chain 1|2|4 [float16|float32|bfloat16|uint8] [repeats=20] [warmup=3] [files=4096]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
READ_BYTES = {1: 2.05e9 / 4096, 2: 131072 + 2 * 65536, 4: 32768 + 2 * 32768}      # the last kernel's input a file


def main():
    import numpy as np
    import torch
    import nhwcodec_amd as na
    mode, scale = sys.argv[1], int(sys.argv[2])
    dtype_name = sys.argv[3] if len(sys.argv) > 3 else "float16"
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    warmup = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    n = int(sys.argv[6]) if len(sys.argv) > 6 else 4096
    assert mode in ("bytes", "fused", "chain") and scale in (1, 2, 4)
    dtype = torch.uint8 if mode == "bytes" else getattr(torch, dtype_name)
    enc = na.Encoder(0, n, device_only=True)
    files, sizes, status = enc.encode_device(enc.synth_device(n, 0), 20)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    enc.close()
    dec = na.Decoder(0, n)
    offs = torch.arange(n, dtype=torch.int64, device="cuda") * na.OUT_STRIDE
    side = 512 // scale
    px = torch.empty((n, side, side, 3), dtype=torch.uint8, device="cuda") if mode != "fused" else None
    out = torch.empty((n, 3, side, side), dtype=dtype, device="cuda") if mode != "bytes" else None
    if mode == "fused":
        fmt = na.TensorFormat(dtype, "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    if mode == "chain":
        sc = (np.float32(1) / (np.float32(255) * np.array(STD, np.float32)))
        bi = -np.array(MEAN, np.float32) / np.array(STD, np.float32)
        sc_t = torch.from_numpy(sc).to("cuda", dtype).view(1, 3, 1, 1)
        bi_t = torch.from_numpy(bi).to("cuda", dtype).view(1, 3, 1, 1)

    def call():
        if mode == "fused":
            return dec.decode_tensor_device(files, offs, sizes, fmt, scale=scale, out=out)[1]
        _, st, _ = dec.decode_scaled_device(files, offs, sizes, scale, px)
        if mode == "chain":
            out.copy_(px.flip((1, 3)).permute(0, 3, 1, 2))
            out.mul_(sc_t).add_(bi_t)
        return st

    stream = torch.cuda.Stream()
    rows = []
    with torch.cuda.stream(stream):
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = call()
            e1.record()
            torch.cuda.synchronize()
            t = dec.timing()
            if i >= warmup:
                rows.append((e0.elapsed_time(e1), t.total_ms, t.recon_ms))
    assert int(st.abs().sum()) == 0
    med = lambda k: sorted(r[k] for r in rows)[len(rows) // 2]
    line = {"mode": mode, "scale": scale, "dtype": str(dtype).replace("torch.", ""), "files": n, "quality": 20, "repeats": repeats, "warmup": warmup,
            "call_ms": {"median": round(med(0), 4), "min": round(min(r[0] for r in rows), 4), "max": round(max(r[0] for r in rows), 4)},
            "decoder_total_ms": round(med(1), 4), "recon_ms": round(med(2), 4)}
    if mode != "chain":
        per_file = READ_BYTES[scale] + 3 * side * side * dtype.itemsize
        line["last_kernel_bytes_per_file"] = int(per_file)
        line["last_kernel_TBps_by_recon_ms"] = round(n * per_file / (med(2) * 1e-3) / 1e12, 2)
    print(json.dumps(line))
    dec.close()


if __name__ == "__main__":
    main()
