"""The Green-Gauss gradient as a differentiable PyTorch op: ``green_gauss(var, part)``.

forward  = the gradient kernel of the partition (cfdp_gpu_gradients),
backward = its adjoint (cfdp_gpu_gradients_adjoint, csrc/gg_adjoint.hip): vbar = A^T gbar.

One partition, ``with_exchange = 0`` semantics: the op maps ``var`` [nall][7] (float64, on the partition's device, FILE
numbering) to ``grad`` [nall][7][3], whose ghost rows are 0 (no kernel computes them).  The ghost rows of ``var`` enter as
constants -- they are detached, no gradient flows to them -- which is the transpose the adjoint kernel computes (the
partition's own map var_own -> grad_own).  On an unpartitioned mesh (nall == nown) that is the whole operator.

Everything stays on the device: torch reads and writes the context's own buffers in place (they are handed to torch through
``__cuda_array_interface__``, no copy), renumbering to tile order (new2old) and decoding the stored form of the gradient
rows (csrc/gg_kernels.h: gg_a_decode) are torch indexing and arithmetic.

Streams: the kernels run on the context's OWN main stream, synchronised with torch's current stream by events in both
directions around each launch -- the main stream waits for the indexing that filled the context's buffers, torch's stream
waits for the kernel before it reads the result.  (Not torch's stream itself: that is the null stream by default, which
the ABI cannot be handed -- a NULL stream argument means the context's own -- and which the context's non-blocking streams
are not ordered with.)
"""
from __future__ import annotations

import numpy as np
import torch

from . import NGRAD, TILES_ALL, GpuPartition


class _DeviceBuffer:
    """a device buffer of the context as torch sees it (no copy; the context owns the memory)"""

    def __init__(self, ptr: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class _Views:
    """per partition and device: the context's buffers as tensors, and the numbering"""

    def __init__(self, part: GpuPartition, device: torch.device):
        c = part.counts()
        self.nown, self.nall = c["nown"], c["nall"]
        self.device = device
        self.main = torch.cuda.ExternalStream(part.stream(0), device=device)
        n2o = np.ascontiguousarray(part.new2old(), np.int64)
        self.n2o = torch.from_numpy(n2o).to(device)             # [nall] device -> file numbering
        self.n2o_own = self.n2o[: self.nown]
        self.var = self.view(part.lib.cfdp_gpu_var_ptr(part.h), (self.nall, 8))  # slot 7: the dual volume (kept)
        gbar, vbar = part.adjoint_ptrs()
        self.gbar = self.view(gbar, (self.nall, 21))
        self.vbar = self.view(vbar, (self.nown, NGRAD))
        # owned points without faces: the gradient kernel leaves their rows alone; the op's rows there are 0
        deg = np.bincount(np.asarray(part.dom.fpoint).ravel(), minlength=self.nall)[n2o[: self.nown]]
        self.faceless = torch.from_numpy(np.flatnonzero(deg == 0)).to(device)

    def view(self, ptr: int, shape) -> torch.Tensor:
        return torch.as_tensor(_DeviceBuffer(ptr, shape), device=self.device)

    def grad_rows(self, part: GpuPartition) -> torch.Tensor:
        """the owned rows of the current grad buffer, decoded: [nown][21], device numbering"""
        nown, nghost = self.nown, self.nall - self.nown
        g = self.view(part.grad_ptr(), (self.nall * 21,))  # [A1: nown x 6][ghost: nghost x 21][A2: nown x 4][B: nown x 11]
        a1 = g[: nown * 6].view(nown, 6)
        o = nown * 6 + nghost * 21
        a2 = g[o: o + nown * 4].view(nown, 4)
        b = g[o + nown * 4: o + nown * 15].view(nown, 11)
        first = torch.stack([a1[:, 0], a1[:, 3] - a2[:, 0], a1[:, 4] - a2[:, 1], a2[:, 0], a1[:, 1],
                             a1[:, 5] - a2[:, 2], a2[:, 1], a2[:, 2], a1[:, 2], a2[:, 3]], 1)  # gg_a_decode
        rows = torch.cat([first, b], 1)
        if self.faceless.numel():
            rows[self.faceless] = 0.0
        return rows


def _views(part: GpuPartition, device: torch.device) -> _Views:
    v = getattr(part, "_torch_views", None)
    if v is None or v.device != device:
        v = _Views(part, device)
        part._torch_views = v
    return v


def _after_main(v: _Views) -> None:
    """torch's current stream waits for the context's main stream (whatever ran there before may still read the buffers
    the op is about to fill)"""
    ev = torch.cuda.Event()
    ev.record(v.main)
    torch.cuda.current_stream(v.device).wait_event(ev)


class _OnMain:
    """the kernel goes to the context's main stream, between two event waits: the main stream waits for what torch's
    current stream has enqueued so far (the indexing that filled the buffers), and torch's current stream waits for the
    kernel before it reads the result"""

    def __init__(self, v: _Views):
        self.v = v

    def __enter__(self):
        self.cur = torch.cuda.current_stream(self.v.device)
        ev = torch.cuda.Event()
        ev.record(self.cur)
        self.v.main.wait_event(ev)
        return self

    def __exit__(self, *exc) -> None:
        ev = torch.cuda.Event()
        ev.record(self.v.main)
        self.cur.wait_event(ev)


class _GreenGauss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, own: torch.Tensor, ghost: torch.Tensor, part: GpuPartition) -> torch.Tensor:
        v = _views(part, own.device)
        ctx.part = part
        _after_main(v)
        v.var[:, :NGRAD] = torch.cat([own, ghost])[v.n2o]
        with _OnMain(v):
            part.gradients(TILES_ALL)
        out = torch.zeros(v.nall, NGRAD * 3, dtype=torch.float64, device=own.device)
        out[v.n2o_own] = v.grad_rows(part)
        return out.view(v.nall, NGRAD, 3)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        part = ctx.part
        v = _views(part, gout.device)
        _after_main(v)
        v.gbar[: v.nown] = gout.reshape(v.nall, NGRAD * 3)[v.n2o_own]
        with _OnMain(v):
            part.gradients_adjoint()
        gown = torch.empty(v.nown, NGRAD, dtype=torch.float64, device=gout.device)
        gown[v.n2o_own] = v.vbar
        return gown, None, None


def green_gauss(var: torch.Tensor, part: GpuPartition) -> torch.Tensor:
    """grad [nall][7][3] = the Green-Gauss gradient of var [nall][7] (float64, on the partition's device, file numbering)
    on partition `part`; differentiable in the OWNED rows of var (ghost rows are constants; module docstring)"""
    c = part.counts()
    nown, nall = c["nown"], c["nall"]
    if var.dtype != torch.float64 or var.dim() != 2 or tuple(var.shape) != (nall, NGRAD):
        raise ValueError(f"var must be a float64 [{nall}][{NGRAD}] tensor, not {var.dtype} {list(var.shape)}")
    if var.device.type != "cuda" or var.device.index != part.lib.cfdp_gpu_device(part.h):
        raise ValueError(f"var must live on the partition's device (cuda:{part.lib.cfdp_gpu_device(part.h)}), not {var.device}")
    return _GreenGauss.apply(var[:nown], var[nown:].detach(), part)
