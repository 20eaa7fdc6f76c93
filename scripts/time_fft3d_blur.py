"""fft3d_from2d on two resident 50 x 2048 x 2048 uint16 stacks: the blur-normalised chain (gb=5) beside the plain one
(gb=0) in one process; median ms of 10 calls after 3 warm-ups and the kernel time of the parts (developer tool).
The target is the source rolled by a known shift, so the printed shifts check themselves."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from imageanalysis3_amd import _lib as L
from imageanalysis3_amd.alignment_tools import fft3d_from2d
shape = (50, 2048, 2048)
rng = np.random.default_rng(5)
ref = (400.0 + 15.0 * rng.standard_normal(shape, dtype=np.float32)).astype(np.uint16)
src = np.roll(ref, (1, -5, 7), axis=(0, 1, 2))
lib = L.lib(); L.check(lib.ia3_init(0))
a, b = L.DeviceStack.upload(src), L.DeviceStack.upload(ref)
del src, ref
for gb in (0, 5):
    for _ in range(3):
        t = fft3d_from2d(a, b, gb=gb, max_disp=150)
    ms = []
    for _ in range(10):
        L.check(lib.ia3_sync()); t0 = time.perf_counter()
        t = fft3d_from2d(a, b, gb=gb, max_disp=150)
        ms.append((time.perf_counter() - t0) * 1e3)
    L.profile_enable(True); L.profile_collect()
    for _ in range(5):
        fft3d_from2d(a, b, gb=gb, max_disp=150)
    L.check(lib.ia3_sync()); prof = L.profile_collect(); L.profile_enable(False)
    print("gb=%d: median %.3f ms (min %.3f, max %.3f) per fft3d_from2d, shift %s; kernels per call: %s" % (
        gb, np.median(ms), min(ms), max(ms), t, {k: round(v[1] / 5, 3) for k, v in prof.items()}), flush=True)
a.free(); b.free()
