"""What the test modules share that belongs to no one feature: where things are, how a command-line tool and the library are brought up, the
committed decoder files, and a few comparisons.  The per-topic helpers are in picture_cases.py, tensor_cases.py, enc_stages.py and dec_stages.py."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEC_GOLD = os.path.join(ROOT, "tests", "golden", "dec")                # the committed .nhw files, one or two a quality
CLI = os.path.join(ROOT, "tools", "nhw-enc")
DEC_CLI = os.path.join(ROOT, "tools", "nhw-dec")
CANARY = 0xA5                                                          # the byte a buffer is filled with where nothing may be written


def run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def built_cli(name):
    """the path of tools/<name> (nhw-enc, nhw-dec), made first if it is missing"""
    exe = os.path.join(ROOT, "tools", name)
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools")])
    return exe


def load_lib():
    """libnhwhip.so, built first if it is missing, as a handle of the caller's own with load_library()'s prototypes.  load_library() imports
    torch first: a process must have one HIP runtime, and a test module's GPU tests follow its others in the same process -- a bare
    ctypes.CDLL in front of torch brings in the system's runtime, and then neither finds a device."""
    import nhwcodec_amd
    if not os.path.exists(nhwcodec_amd.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return nhwcodec_amd.load_library()


def golden(name):
    with open(os.path.join(DEC_GOLD, name), "rb") as f:
        return f.read()


def golden_names():
    return sorted(n for n in os.listdir(DEC_GOLD) if n.endswith(".nhw"))


def device_arena(files):
    """files -> (arena, offsets, lengths) on the device, as decode_device takes them"""
    import torch
    offs = np.zeros(len(files), np.int64)
    offs[1:] = np.cumsum([len(f) for f in files])[:-1]
    blob = np.frombuffer(b"".join(files) + bytes(64), np.uint8).copy()
    return (torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(np.array([len(f) for f in files], np.int32)).cuda())


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-9))


def same_files(a, b, sizes):
    """two device arenas of one file a row hold the same bytes within every row's size"""
    import torch
    mask = torch.arange(a.shape[1], device="cuda")[None, :] < sizes.long()[:, None]
    return not bool(((a != b) & mask).any())
