"""time of one pass of the gradient's adjoint (csrc/gg_adjoint.hip) against the gradient kernel on the same plan: the 64^3
lattice, the irregular stand-in (64^3 points, CONN_IRREGULAR, scrambled numbering) and 128^3.  Both event-timed on the
context's main stream, back-to-back launches, after a warm-up; median of 7 batches.  frac = algo_bytes_adjoint at 8 TB/s
over the measured time.  Prints one JSON line.
    python tools/adjoint_probe.py [lattice64 irregular64 lattice128]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

m = load_package()
MESHES = {"lattice64": (64, {}), "irregular64": (64, dict(connectivity=m.CONN_IRREGULAR, numbering=1)), "lattice128": (128, {})}


def timed(part, fn, iters):
    st = torch.cuda.ExternalStream(part.stream(0), device=torch.device("cuda", 0))
    for _ in range(iters):  # warm-up (clocks, caches)
        fn()
    out = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        for _ in range(iters):
            fn()
        b.record(st)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


rows = []
for name in sys.argv[1:] or list(MESHES):
    n, kw = MESHES[name]
    dom = m.gen_domain(m.gen_params(n, ndomains=1, **kw), 0)
    m.fill_var(dom, None, m.VAR_HASH)
    part = m.GpuPartition(dom)
    part.set_grad_adjoint(np.random.default_rng(1).standard_normal((dom.nall, 7, 3)))
    iters = 100 if n <= 64 else 30
    adj = timed(part, part.gradients_adjoint, iters)
    grad = timed(part, part.gradients, iters)
    forms = m.kernel_forms()  # (switches the log on)
    part.gradients()
    forms = m.kernel_forms()
    nbytes = m.algo_bytes_adjoint(dom.nfaces, dom.nown, dom.nall - dom.nown)
    rows.append(dict(mesh=name, points=dom.nown, faces=dom.nfaces, tiles=part.stats["ntiles"],
                     us_adjoint=round(adj[0], 2), us_adjoint_min_max=[round(adj[1], 2), round(adj[2], 2)],
                     us_gradient=round(grad[0], 2), gradient_forms=forms, ratio_to_gradient=round(adj[0] / grad[0], 3),
                     algo_bytes_adjoint=nbytes, frac_of_8TBs=round(nbytes / (adj[0] * 1e-6) / 8e12, 3)))
    part.close()
    dom.free()
print(json.dumps({"adjoint_probe": rows}))
