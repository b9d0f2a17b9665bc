#!/usr/bin/env python3
"""Developer tool: time ops.rotate_volume at N = 200 000 with the library given as argv[1] (default: the in-tree build);
argv[2], if given, is a build label and adds one JSON line (median / min / max of the ten launches, in us)."""
import importlib, json, os, sys, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ahv = importlib.import_module("3dahv_amd")
if len(sys.argv) > 1:
    ahv._lib.LIB_PATH = os.path.abspath(sys.argv[1])
ops = ahv.ops
dev = torch.device("cuda:0")
N = 200_000
R = ops.so3_grid(N, dev)
v = (torch.randn(1, 16, 8, 8, 8, generator=torch.Generator().manual_seed(0)) * 1.15).to(dev)
src = v[0][None].expand(N, -1, -1, -1, -1)
out = ops.rotate_volume(src, R)
for _ in range(3):
    ops.rotate_volume(src, R)
torch.cuda.synchronize()
ts = []
for _ in range(10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); ops.rotate_volume(src, R); e1.record(); torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
ts.sort()
print("%s: rotate_volume N=%d  min %.4f  median %.4f ms  -> %.2f TB/s (32 804 B per hypothesis)" % (
    os.path.basename(os.path.dirname(ahv._lib.LIB_PATH)), N, ts[0], ts[5], N * 32804 / ts[5] / 1e9))
if len(sys.argv) > 2:
    print(json.dumps({"tool": "rot_time.py", "row": "rotate_volume", "N": N, "build": sys.argv[2], "us": round(1e3 * ts[5], 3),
                      "min_us": round(1e3 * ts[0], 3), "max_us": round(1e3 * ts[-1], 3), "launches": len(ts),
                      "device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__}))
