"""The encoder's stage checks, shared by test_luma_loop.py, test_chroma_loops.py, test_filterbank_gate.py, test_quant_marks.py, test_luma_stream.py,
test_stream_stage.py and test_gpu_parity.py (dec_stages.py is the decoder's counterpart): the workspace buffers by name, the hook that
writes the luma planes, runs one form of nhw_stage_luma_loop (include/nhw_hip_debug.h) and reads them back, the generator images a quality
is tested on and the oracle's files of a batch."""
import ctypes
import os
import re
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from tests.support import ROOT

Q = 65536
N_IMAGES = 64


def ws_index(name):
    """index of a workspace buffer (nhwcodec_amd/csrc/nhw_ws.h, the B_* list) for nhw_debug_read / nhw_debug_write"""
    txt = open(os.path.join(ROOT, "nhwcodec_amd", "csrc", "nhw_ws.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt[txt.index("enum {"):txt.index("B_COUNT")], flags=re.S)
    return re.findall(r"B_[A-Z0-9_]+", body).index("B_" + name)


B_JPEG, B_PROC, B_LL1, B_L2SAVE = (ws_index(n) for n in ("JPEG", "PROC", "LL1", "L2SAVE"))
B_CPROC, B_CLL1, B_CL2SAVE = (ws_index(n) for n in ("CPROC", "CLL1", "CL2SAVE"))
PLANES = (("jpeg", B_JPEG, 8 * Q), ("proc", B_PROC, 8 * Q), ("ll1 + the cell behind", B_LL1, 2 * Q + 2), ("l2save", B_L2SAVE, 2 * Q))


def synthetic_images(q, n=N_IMAGES, first=61000, step=89):
    """n generator images of quality q's own seeds: the luma tests' (chroma_images: the chroma tests')"""
    from oracle.oraclepy import Oracle
    o = Oracle()
    return np.stack([o.synth(first + step * q + i) for i in range(n)])


def chroma_images(q, n=N_IMAGES):
    return synthetic_images(q, n, 52000, 97)


def _want(args):
    from oracle.oraclepy import Oracle
    q, compat, imgs = args
    o = Oracle()
    o.set_oob_mode(bool(compat))
    try:
        return [o.encode(im, q) for im in imgs]
    finally:
        o.set_oob_mode(False)


def oracle_files(imgs, q, compat=False):
    step = 4
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        return [f for part in ex.map(_want, [(q, compat, imgs[i:i + step]) for i in range(0, len(imgs), step)]) for f in part]


class Hook:
    def __init__(self, n):
        import nhwcodec_amd
        self.n = n
        self.e = nhwcodec_amd.Encoder(0, max_batch=n)

    def read(self, buf, i, nbytes):
        out = np.empty(nbytes, np.uint8)
        assert self.e.lib.nhw_debug_read(self.e.h, buf, i, ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(nbytes)) == 0
        return out.view(np.int16)

    def write(self, buf, i, a):
        a = np.ascontiguousarray(a)
        assert self.e.lib.nhw_debug_write(self.e.h, buf, i, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0

    def planes(self):
        return [[self.read(buf, i, nbytes) for _, buf, nbytes in PLANES] for i in range(self.n)]

    def run(self, form, inputs):
        """inputs: per image (jpeg, proc, ll1, l2save) as int16 arrays, written before the launches"""
        import torch
        for i, planes in enumerate(inputs):
            for (_, buf, nbytes), a in zip(PLANES, planes):
                self.write(buf, i, a.ravel()[:min(a.size, nbytes // 2 if buf != B_LL1 else Q)])   # (the cell behind ll1 is left as it stands)
        assert self.e.lib.nhw_stage_luma_loop(self.e.h, self.n, form, None) == 0, "nhw_stage_luma_loop"
        torch.cuda.synchronize()
        return self.planes()


def compare(tag, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        for (name, _, _), a, b in zip(PLANES, g, w):
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, f"{tag} image {i} {name}: {bad.size} cells differ, first {bad[:8].tolist()}"
