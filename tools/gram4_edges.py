#!/usr/bin/env python3
"""tools/gram4_edges.sh run: cfg3 uniform text through the stamped library (abtmp/g4edges/libdaachorse_amd.so, or the one DAAC_EDGES_LIB names).
usage: gram4_edges.py [mib] [launches] [option=value ...]
Per launch: the waves' and the CUs' finish times (a workgroup is a CU's only one: its LDS fills the CU), the CU-time idle between a CU's
last wave and the kernel's end, the time from entry to the first step's text."""
import ctypes as C
import importlib.util
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
variant = os.path.abspath(os.environ.get("DAAC_EDGES_LIB", os.path.join(R, "abtmp", "g4edges", "libdaachorse_amd.so")))
# The stamped library is loaded by path and the project's own library is left where it is (a run that is killed leaves nothing behind):
# the package's loader takes its path from daachorse_amd._build.LIB_PATH, so that module is put in place first with the variant's path.
spec = importlib.util.spec_from_file_location("daachorse_amd._build", os.path.join(R, "daachorse_amd", "_build.py"))
_build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(_build)
_build.LIB_PATH = variant
sys.modules["daachorse_amd._build"] = _build

import numpy as np
import torch

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, _ffi, synth

L = _ffi.lib()
assert os.path.samefile(L._name, variant), L._name
L.daac_g4_edges.argtypes = [C.c_void_p]
args = [x for x in sys.argv[1:] if "=" not in x]
mib = int(args[0]) if args else 4096
launches = int(args[1]) if len(args) > 1 else 3
for kv in sys.argv[1:]:
    if "=" in kv:
        k, v = kv.split("=")
        da.set_option(k, int(v))
pma = da.DoubleArrayAhoCorasick.new(synth.patterns_cfg3())
pma.upload(0)
hay = torch.empty(mib << 20, dtype=torch.uint8, device="cuda")
synth.device_uniform(hay, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
res = torch.zeros(3, dtype=torch.int64, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
ncu = torch.cuda.get_device_properties(0).multi_processor_count
buf = torch.zeros(ncu * 2 * 16 * 8, dtype=torch.int64, device="cuda")
assert L.daac_g4_edges(buf.data_ptr()) == 0
run = lambda: pma.count(ScanMode.FindOverlapping, hay, engine=Engine.Gram, stream=stream, result_dev=res.data_ptr())
for _ in range(5):
    run()
torch.cuda.synchronize()
print(f"cfg3 uniform, {mib} MiB, {da.last_kernel()}, options {[x for x in sys.argv[1:] if '=' in x]}; times in us (wall_clock64, 100 MHz) from the first wave's entry")
q = lambda a: "min %8.1f  median %8.1f  p99 %8.1f  max %8.1f" % (a.min(), np.median(a), np.percentile(a, 99), a.max())
for it in range(launches):
    buf.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    b = buf.cpu().numpy().reshape(-1, 8)
    b = b[b[:, 0] != 0]
    t0 = b[:, 0].min()
    entry, first, done, exit_ = [(b[:, i] - t0) / 100.0 for i in range(4)]
    first = np.where(b[:, 1] == 0, entry, first)   # (a wave without a region)
    end = exit_.max()
    nw = len(b)
    wpb = 16
    cu_done = done.reshape(-1, wpb).max(axis=1)
    cu_exit = exit_.reshape(-1, wpb).max(axis=1)
    xcc = (b[:, 5] & 0xf).reshape(-1, wpb)[:, 0]
    print(f"launch {it}: count {int(res[0].item())}, HIP events around the call {e0.elapsed_time(e1) * 1e3:.1f} us, stamps: first entry to last exit {end:.1f} us, {nw} waves, {nw // wpb} workgroups")
    print(f"  wave entry                      {q(entry)}")
    print(f"  entry -> first step's text      {q(first - entry)}   (from the first wave's entry: {q(first)})")
    print(f"  wave: last region finished      {q(done)}")
    print(f"  CU: its last wave finished      {q(cu_done)}")
    print(f"  idle wave-time before the end   {100.0 * (end - done).sum() / (nw * end):.2f} % of waves x kernel time")
    print(f"  idle CU-time before the end     {100.0 * (end - cu_done).sum() / (len(cu_done) * end):.2f} % of CUs x kernel time   (by the CU's exit stamp: {100.0 * (end - cu_exit).sum() / (len(cu_exit) * end):.2f} %)")
    print("  CU finish by XCC_ID             " + "  ".join(f"{x}: median {np.median(cu_done[xcc == x]):.1f} max {cu_done[xcc == x].max():.1f}" for x in sorted(set(xcc.tolist()))))
