"""Developer tool (GPU box): what an encode straight from a training tensor costs.  Recorded, not gated.
`files` generator images (seeds 0 ..) as a float32 [n, 3, 512, 512] RGB, top-down tensor under the ImageNet mean and std (what
decode_tensor_device stores for them), encoded at q20 on ONE handle and one torch stream under the inverted format: `warmup` calls that do not
count, then `repeats` calls, each between two events of that stream.
  bytes    (a) encode_device on the ready bytes
  tensor   (b) encode_tensor_device
  chain    (c) torch's flip, permute, affine, round, clamp, to(uint8), contiguous, then encode_device
  kernel   tensor_to_bytes_device alone: k_tensor_to_bytes<f32, CHW> moves 15 bytes a pixel (12 read, 3 written), and the TB/s that makes of
           its time, to be held against the 5.5 TB/s device-copy rate bench.py reports
Prints one JSON line with median / min / max ms of each, after checking that (b) and (c) produce (a)'s files.
usage: python tools/dev/tensor_encode_time.py [repeats=7] [warmup=2] [files=4096]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    import numpy as np
    import torch
    import nhwcodec_amd as na
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    enc = na.Encoder(0, n, device_only=True)
    px = enc.synth_device(n, 0)
    dec_fmt = na.TensorFormat("float32", "CHW", "RGB", "reversed", mean=MEAN, std=STD)
    fmt = dec_fmt.inverted()
    x = torch.empty((n, 3, 512, 512), dtype=torch.float32, device="cuda")
    x.copy_(px.flip((1, 3)).permute(0, 3, 1, 2))
    x.mul_(torch.tensor(dec_fmt.scale, device="cuda").view(1, 3, 1, 1)).add_(torch.tensor(dec_fmt.bias, device="cuda").view(1, 3, 1, 1))
    sc, bi = torch.tensor(fmt.scale, device="cuda"), torch.tensor(fmt.bias, device="cuda")
    out = enc.alloc_out(n)
    torch.cuda.synchronize()
    assert torch.equal(na.tensor_to_bytes_device(x, fmt), px), "the tensor does not convert back to the generator's bytes"

    def chain():
        b = x.flip((1, 2)).permute(0, 2, 3, 1).mul(sc.flip(0)).add(bi.flip(0)).round().clamp(0, 255).to(torch.uint8).contiguous()   # (the constants by byte channel)
        return enc.encode_device(b, 20, out=out)

    calls = {"bytes": lambda: enc.encode_device(px, 20, out=out), "tensor": lambda: enc.encode_tensor_device(x, fmt, 20, out=out), "chain": chain,
             "kernel": lambda: na.tensor_to_bytes_device(x, fmt)}
    res = {"files": n, "repeats": repeats, "warmup": warmup}
    want = None
    for name, call in calls.items():
        ms = []
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
        if name != "kernel":
            sizes, status = out[1].cpu().numpy(), out[2].cpu().numpy()
            assert not status.any()
            digest = (sizes.tolist(), int(sum(int(out[0][i, :int(sizes[i])].to(torch.int64).sum()) for i in range(0, n, max(1, n // 64)))))
            want = want or digest
            assert digest == want, f"{name}: other files than the byte encode"
        res[name + "_ms"] = [round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)]
    res["kernel_bytes"] = n * 512 * 512 * 15
    res["kernel_TBps"] = round(res["kernel_bytes"] / (res["kernel_ms"][0] * 1e-3) / 1e12, 3)
    print(json.dumps(res))
    enc.close()


if __name__ == "__main__":
    main()
