"""BP 64 (three workgroups per CU where the halo fits the 26,624-byte tier) against the table's BP 128 for
every 'x6h:' plan entry that has BP 128 and whose BP 64 launch reaches that tier, at the entry's own split
count (BP does not change the order of an element's sums, split-K does), alternated in one process.
Prints one JSON line per entry; bp64_wins where BP 64's slowest timing beats BP 128's fastest by more than
BP 128's spread (profiles/x6h_residency_r11.txt, session 4).

    python scripts/halo_bp_probe.py
"""
import json, sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from ddl25spring_amd.ops import functional_f32 as F32
from ddl25spring_amd.ops.functional import ConvGeom
from halo_plan_probe import timed

dev = torch.device("cuda")
F32.ensure_workspace(dev)
plans = json.load(open(F32._TUNED_PATH))["plans"]
modes = {"fwd": F32.F_FWD, "dgrad": F32.F_DGRAD}
for key, p in plans.items():
    if not key.startswith("x6h:") or p[0] != 128:
        continue
    _, mname, geo = key.split(":")
    g = ConvGeom(*map(int, geo.split(",")))
    mode = modes[mname]
    lay = F32.halo_layout(mode, g, 64)
    if lay is None or lay["tier"] != F32.HALO_TINY:
        continue
    x = torch.randn(g.G, g.N, g.H, g.W, g.C, device=dev)
    w = torch.randn(g.G, g.K, g.R, g.S, g.C, device=dev) * 0.05
    dy = torch.randn(g.G, g.N, g.P, g.Q, g.K, device=dev)
    run = (lambda: F32.conv_fwd(x, w, g, stats=F32.SlotStats())) if mode == F32.F_FWD else (lambda: F32.conv_dgrad(dy, w, g))
    res = {64: [], 128: []}
    for rnd in range(4):
        for bp in (128, 64):
            F32.set_plan(mode, g, bp, 128, int(p[2]), "x6h")
            t = timed(run, 40) * 1e3
            if rnd:  # the first round warms up
                res[bp].append(round(t, 1))
    F32.clear_plan(mode, g)
    a, b = res[128], res[64]
    win = min(a) - max(b) > max(a) - min(a)
    print(json.dumps(dict(key=key, split=p[2], bp128_us=a, bp64_us=b, bp64_wins=win)), flush=True)
    del x, w, dy
