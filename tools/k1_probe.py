#!/usr/bin/env python3
"""K1 at cfg-3 size: stage time per call (HIP events of the library).  python tools/k1_probe.py [F lmax]
(an A/B build of the library - `make ab` in cora_amd/csrc - is selected with CORAHIP_LIB=cora_amd/libcorahip_<TAG>.so)."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cora_amd import _lib
from cora_amd.parallel import SkyShard
from cora_amd.signal import corr21cm
ctx = _lib.get_context()
F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
lmax = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
freq = 400.0 + (np.arange(F) + 0.5) * (400.0 / F)
sh = SkyShard(corr21cm.Corr21cm(), freq, 64, lmax, zromb=3, ctx=ctx)
for _ in range(3):
    C = sh._clarray_local()
torch.cuda.synchronize()
ctx.profile_reset(); ctx.profile_enable(True)
for _ in range(10):
    C = sh._clarray_local()
torch.cuda.synchronize()
ctx.profile_enable(False)
ms, n = ctx.profile_get("clarray")
print("clarray %.3f ms per call (%d calls)" % (ms / n, n))
