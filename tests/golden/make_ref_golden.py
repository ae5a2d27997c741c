"""Records what the REAL reference (oracle/_ref: the unmodified sources behind the zero-guard shims, and the stock binaries) answers to
the inputs of the tests that compare against it, so that those tests run from the repository alone.

Run where the reference's sources have produced oracle/_ref (`make -C oracle/ref`):
    python tests/golden/make_ref_golden.py
Output (data only -- inputs are regenerated from integer seeds, outputs are hashes of the reference's bytes):
    tests/golden/ref_record.json
        trace      <input>_q<q>: sha256 of the .nhw file + the short hash of every checkpoint blob, in call order
        colour     <input>_q<q>: the first checkpoint (downsample_YUV420) and the short hashes of its Y, U, V planes
        decode     <input>_q<q>: sha256 of the reference encoder's file, of the reference decoder's Y/U/V planes and of its BMP
        ref_decodes_oracle_file: the oracle's q20 file of synth seed 4 and the BMP the stock nhw-dec writes from it
        stock      q<q> / <input>: the stock nhw-enc's file as length, un-initialised positions and sha256 of the other bytes
        codebook   the fuzz picture's sha256 and the reference's file sha256 per quality (null: the reference exited with -1)
        cli        the stock nhw-enc / nhw-dec answers (exit code, stdout lines, stderr) to the tests' command lines and bad BMPs
The cases are the tests' own (tests/test_oracle.py, tests/test_decode.py, tests/test_dist_cli.py); every record is checked against the
oracle before it is written, so a record never pins a disagreement.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "dev"))
from oracle.harness import RefDecoder, RefEncoder, class_image, stock_encode, uninitialised_positions  # noqa: E402
from oracle.oraclepy import Oracle  # noqa: E402
from tests import test_decode as td, test_dist_cli as tc, test_oracle as to  # noqa: E402


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def run(exe, *a):
    p = subprocess.run([exe, *a], capture_output=True, text=True)
    return p.returncode, p.stdout, p.stderr


def main():
    ref, rd, orc = RefEncoder(), RefDecoder(), Oracle()
    rec = {"trace": {}, "colour": {}, "decode": {}, "stock": {}, "codebook": {}, "cli": {}}

    def trace(key, img, q):
        data, tr = ref.encode(img, q, trace=True)
        r = to._trace_record(data, tr)
        to._assert_trace(r, *orc.encode(img, q, trace=True), key)
        rec["trace"][key] = r

    for q in to.TRACE_QS:
        trace(f"synth_s12_q{q}", orc.synth(12), q)
    for kind in to.HARD_KINDS:
        for q in to.HARD_QS:
            trace(f"{kind}_s3_q{q}", class_image(kind, 3), q)

    for q in to.COLOUR_QS:
        for name, img in to.colour_images(orc):
            _, tr = ref.encode(img, q, trace=True)
            cp, blobs = tr[0]
            y, u, v = orc.color(img, q)
            assert blobs[:3] == [y.tobytes(), u.tobytes(), v.tobytes()], (name, q)
            rec["colour"][f"{name}_q{q}"] = [cp, [to._h16(b) for b in blobs]]

    cases = [(f"synth_s{seed}_q{q}", q, orc.synth(seed)) for q, seed in td.LIVE_SYNTH]
    cases += [(f"{kind}_s1_q20", 20, class_image(kind, 1)) for kind in td.LIVE_CLASSES]
    for key, q, img in cases:
        nhw = ref.encode(img, q)
        planes, wq = rd.planes(nhw)
        bmp = rd.bmp(nhw)
        got, gq = orc.decode(nhw, planes=True)
        assert nhw == orc.encode(img, q) and wq == gq == q and np.array_equal(planes, got), key
        assert bmp == orc.bmp_header() + orc.decode(nhw)[0].tobytes(), key
        rec["decode"][key] = {"quality": wq, "nhw_sha256": sha(nhw), "planes_sha256": sha(np.ascontiguousarray(planes).tobytes()),
                              "bmp_sha256": sha(bmp)}

    nhw = orc.encode(orc.synth(4), 20)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "a.nhw")
        with open(p, "wb") as fh:
            fh.write(nhw)
        subprocess.check_call([tc.REF_DEC_CLI, p, os.path.join(d, "a.bmp")], stdout=subprocess.DEVNULL)
        with open(os.path.join(d, "a.bmp"), "rb") as fh:
            bmp = fh.read()
    assert bmp == orc.bmp_header() + orc.decode(nhw)[0].tobytes()
    rec["ref_decodes_oracle_file"] = {"nhw_sha256": sha(nhw), "bmp_sha256": sha(bmp)}

    orc.set_oob_mode(True)
    try:
        for q in to.STOCK_QS:
            rec["stock"][f"q{q}"] = {}
            for name, img in to.stock_images(orc, q):
                runs = [stock_encode(img, q) for _ in range(2)]      # the un-initialised bytes may change from run to run; the rest may not
                pad = sorted(uninitialised_positions(runs[0]))
                r = {"len": len(runs[0]), "pad": pad, "masked_sha256": to.masked_sha(runs[0], pad)}
                got = orc.encode(img, q)
                assert len(runs[1]) == len(got) == r["len"] and to.masked_sha(runs[1], pad) == to.masked_sha(got, pad) == r["masked_sha256"], (q, name)
                rec["stock"][f"q{q}"][name] = r
    finally:
        orc.set_oob_mode(False)

    from gpu_fuzz_classes import make
    img = make(to.CODEBOOK_SEED)
    rec["codebook"] = {"image_sha256": sha(img.tobytes()), "nhw_sha256": {}}
    for q in to.CODEBOOK_QS:
        try:
            want = sha(ref.encode(img, q))
        except RuntimeError as ex:
            assert "rc=-1" in str(ex)
            want = None
        rec["codebook"]["nhw_sha256"][str(q)] = want

    cli = rec["cli"] = {"enc_args": {}, "bad_bmp": {}, "dec_args": {}}
    for args in tc.ENC_ARGS:
        rc, out, err = run(tc.REF_CLI, *args)
        cli["enc_args"][" ".join(args)] = {"rc": rc, "stdout_lines": out.splitlines(), "stderr": err}
    with tempfile.TemporaryDirectory() as d:
        for name, data in tc.BAD_BMPS.items():
            p = os.path.join(d, name)
            with open(p, "wb") as fh:
                fh.write(data)
            rc, out, _ = run(tc.REF_CLI, p, os.path.join(d, "r.nhw"))
            cli["bad_bmp"][name] = {"rc": rc, "stdout": out}
    for args in tc.DEC_ARGS:
        rc, out, err = run(tc.REF_DEC_CLI, *args)
        cli["dec_args"][" ".join(args)] = {"rc": rc, "stdout_lines": out.splitlines(), "stderr": err}

    with open(os.path.join(HERE, "ref_record.json"), "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("traces", len(rec["trace"]), "decodes", len(rec["decode"]), "stock files", sum(len(v) for v in rec["stock"].values()))


if __name__ == "__main__":
    main()
