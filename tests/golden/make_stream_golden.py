"""Records what the stream stage answers to the crafted symbol streams of tests/stream_cases.py, pinned to the REAL reference.

Run where the reference's sources have produced oracle/_ref (`make -C oracle ref`):
    python tests/golden/make_stream_golden.py
Output (hashes only -- every stream is regenerated from the case list):
    tests/golden/stream_record.json
        cases      <case name>: a short hash of what the oracle's export (nhwo_stream_stage) returns -- the rewritten luma part, the packet
                   words, both code books, both sign-word arrays and every scalar
        reference  <case name>: "equal" -- the unmodified wavlts2packet (compress_pixel.c:53, behind oracle/ref/ref_shim.c's allocator and
                   zeroed stack) was given the oracle's rewritten stream and returned the same words, books, sign words and sizes;
                   "exit" -- it left through exit(-1) where the oracle answers NHWO_E_CODEBOOK; "over capacity" -- the stream takes more
                   than the 80000 words of the reference's packet block, which it would overrun, so it was not sent there
A case is checked before it is written, so the record never pins a disagreement.  The rewrites sit in the middle of encode_image and
cannot be called alone: for them the oracle's transcription is the reference (pinned on pictures by the pre_highres_compression checkpoint
of tests/test_oracle.py).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.harness import RefEncoder  # noqa: E402
from oracle.oraclepy import Oracle  # noqa: E402
from tests import stream_cases as sc  # noqa: E402

SCALARS = ("size_data1", "size_data2", "size_book1", "size_book2", "tree_end", "select1", "select2", "wavelet_type")
ARRAYS = ("packet", "book1", "book2", "sel_word1", "sel_word2")


def main():
    ref, orc = RefEncoder(), Oracle()
    rec = {"cases": {}, "reference": {}}
    for name, luma, chroma in sc.all_cases(orc):
        sc.admissible(name, luma, chroma)
        assert name not in rec["cases"], name
        r = orc.stream_stage(luma, chroma, 80000)
        rec["cases"][name] = sc.digest(r)
        if r["words"] > 80000:
            rec["reference"][name] = "over capacity"
            continue
        assert r["select1_pre"] < 65536 and r["select2_pre"] < 65536, name     # (unsigned short in the reference)
        rc, g = ref.stream_packet(np.concatenate([r["luma"], chroma]), r["select1_pre"], r["select2_pre"])
        if r["status"] != 0:
            assert r["status"] == -2 and rc == -1, (name, r["status"], rc)
            rec["reference"][name] = "exit"
            continue
        assert rc == 0, (name, rc)
        diff = [k for k in SCALARS if g[k] != r[k]] + [k for k in ARRAYS if not np.array_equal(g[k], r[k])]
        assert not diff, (name, diff)
        rec["reference"][name] = "equal"
    with open(os.path.join(HERE, "stream_record.json"), "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    kinds = list(rec["reference"].values())
    print("cases", len(kinds), {k: kinds.count(k) for k in sorted(set(kinds))})


if __name__ == "__main__":
    main()
