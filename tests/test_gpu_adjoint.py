"""The adjoint of the gradient on an MI355X (csrc/gg_adjoint.hip through the C ABI, the in-process rank group, RCCL, the torch
op) against the numpy statement of tests/adjoint_ref.py.  Criterion: |d| <= 1e-10 * max(|ref|, sum |terms|) per component."""
import os

import numpy as np
import pytest

from adjoint_ref import np_adjoint_scale, np_gradients_adjoint
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-10
LANES = [1, 2, 4, 8]
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))


def check(got, fp, fn, vol, gbar, nown, ghosts=False, strict=True, what=""):
    ref = np_gradients_adjoint(fp, fn, vol, gbar, nown, ghosts)[:nown]
    scale = np.maximum(np.abs(ref), np_adjoint_scale(fp, fn, vol, gbar, nown, ghosts)[:nown])
    scale = np.where(scale > 0, scale, 1.0)
    d = np.abs(got[:nown] - ref)
    assert (d / scale).max() <= TOL, (what, float((d / scale).max()))
    if strict:  # also relative to the value itself wherever it is not a cancelled sum
        big = np.abs(ref) >= 1e-6 * scale
        worst = float((d[big] / np.abs(ref[big])).max()) if big.any() else 0.0
        print(f"{what}: worst |d|/|ref| = {worst:.3e} over {int(big.sum())} components")
        assert worst <= TOL, (what, worst)


def run_adjoint(pkg, dom, gbar, tile_points=0, lanes=4):
    part = pkg.GpuPartition(dom, tile_points=tile_points, grad_lanes=lanes, flux_lanes=lanes)
    part.set_grad_adjoint(gbar)
    part.gradients_adjoint()
    v = part.get_var_adjoint()
    part.close()
    return v


def plain_domain(pkg, fp, fn, vol, nown, var=None):
    return pkg.domain_from_arrays(np.ascontiguousarray(fp, np.int32), fn, vol, nown,
                                  var=var if var is not None else np.ones((len(vol), 7)))


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("tile_points", [16, 64, 128])
def test_adjoint_golden_meshes(gpu, name, lanes, tile_points):
    """every domain of every fixture on its own (ghost gbar = 0: the partition's own transpose), seeded random gbar"""
    pkg = gpu
    fx = load_golden(name)
    rng = np.random.default_rng(sum(name.encode()) + lanes + tile_points)
    for d in range(int(fx["ndomains"])):
        if f"d{d}_fpoint" not in fx.files:
            continue
        fp, fn, vol, nown = fx[f"d{d}_fpoint"], fx[f"d{d}_fnormal"], fx[f"d{d}_pvolume"], int(fx[f"d{d}_nown"])
        gbar = rng.standard_normal((len(vol), 7, 3))
        gbar[nown:] = np.nan  # ghost rows are never read without the exchange
        dom = plain_domain(pkg, fp, fn, vol, nown, fx[f"d{d}_var"])
        v = run_adjoint(pkg, dom, gbar, tile_points, lanes)
        check(v, fp, fn, vol, np.nan_to_num(gbar), nown, what=f"{name} d{d} lanes {lanes} tile {tile_points}")
        dom.free()


@pytest.mark.parametrize("lanes", LANES)
def test_dot_product_identity_with_the_gpu_forward(gpu, lanes):
    """<A var, gbar> == <var, A^T gbar>, both sides computed by the GPU kernels on the same partition"""
    pkg = gpu
    gp = pkg.gen_params(20, 18, 16, ndomains=1)
    dom = pkg.gen_domain(gp, 0)
    rng = np.random.default_rng(lanes)
    dom.var[:] = rng.standard_normal(dom.var.shape)
    var = dom.var.copy()
    part = pkg.GpuPartition(dom, tile_points=64, grad_lanes=lanes, flux_lanes=lanes)
    part.gradients()
    part.pull_fields()
    g = dom.grad.copy()
    gbar = rng.standard_normal(g.shape)
    part.set_grad_adjoint(gbar)
    part.gradients_adjoint()
    v = part.get_var_adjoint()
    part.close()
    lt, rt = g * gbar, var * v
    assert abs(lt.sum() - rt.sum()) <= 1e-12 * max(np.abs(lt).sum(), np.abs(rt).sum())
    dom.free()


def test_adjoint_plan_forms(gpu):
    """irregular generator mesh (hubs of 60+, scrambled numbering, long lists in chunks), a Delaunay mesh, hub points of
    hundreds of faces (a GENERIC launch group; at 1000 leaves the rows no longer fit whole and equations are staged in
    slices), a random multigraph with long lists, small and large tiles, host- and device-built plans"""
    pkg = gpu
    from unstructured import delaunay_mesh
    rng = np.random.default_rng(17)
    cases = []
    irr = pkg.gen_domain(pkg.gen_params(24, 20, 18, ndomains=1, connectivity=pkg.CONN_IRREGULAR, numbering=1), 0)
    cases.append(("irregular", irr.fpoint.copy(), irr.fnormal.copy(), irr.pvolume.copy(), irr.nown))
    irr.free()
    _, fp, fn, vol, _ = delaunay_mesh(12000, seed=5)
    cases.append(("delaunay", fp, fn, vol, len(vol)))
    for nleaf in (300, 1000):
        n = nleaf + 1
        star = np.stack([np.zeros(nleaf, np.int32), np.arange(1, n, dtype=np.int32)], 1)
        chain = np.stack([np.arange(1, n - 1, dtype=np.int32), np.arange(2, n, dtype=np.int32)], 1)
        fp = np.concatenate([star, chain]).astype(np.int32)
        flip = rng.random(len(fp)) < 0.5
        fp[flip] = fp[flip][:, ::-1]
        cases.append((f"hub{nleaf}", fp, rng.standard_normal((len(fp), 3)), rng.uniform(0.5, 2.0, n), n))
    n = 3000
    deg = rng.integers(0, 12, n)
    deg[rng.choice(n, 12, replace=False)] = rng.integers(40, 90, 12)
    ends = np.repeat(np.arange(n), deg)
    rng.shuffle(ends)
    fp = np.stack([ends, rng.integers(0, n, len(ends))], 1).astype(np.int32)
    fp = fp[fp[:, 0] != fp[:, 1]]  # (parallel faces and isolated points stay)
    cases.append(("multigraph", fp, rng.standard_normal((len(fp), 3)), rng.uniform(0.5, 2.0, n), n))
    for name, fp, fn, vol, nown in cases:
        gbar = rng.standard_normal((len(vol), 7, 3))
        for tile_points, lanes, device_plan in ((16, 4, "3"), (64, 8, "3"), (128, 4, "0"), (0, 2, "3")):
            if name.startswith("hub") and tile_points == 16:
                continue
            os.environ["CFDP_PLAN_DEVICE"] = device_plan
            try:
                dom = plain_domain(pkg, fp, fn, vol, nown)
                v = run_adjoint(pkg, dom, gbar, tile_points, lanes)
                dom.free()
            finally:
                os.environ.pop("CFDP_PLAN_DEVICE", None)
            check(v, fp, fn, vol, gbar, nown, what=f"{name} tile {tile_points} lanes {lanes} plan {device_plan}")


def test_adjoint_small_and_large_tiles_in_launches_of_their_own(gpu):
    """a partition whose plan has boundary tiles, two capacity classes and a generic group: each its own launch"""
    pkg = gpu
    from cfd_proxy_amd import multigpu as mg
    gp = pkg.gen_params(20, 16, 12, ndomains=4, connectivity=pkg.CONN_IRREGULAR, numbering=1)
    parts = [mg.build_rank_partition(gp, 4, 2, r, via_files=False)[0] for r in range(2)]
    pkg.merge_link_group(parts)
    p = parts[0]
    rng = np.random.default_rng(2)
    gbar = rng.standard_normal((p.nall, 7, 3))
    g = pkg.GpuPartition(p, tile_points=32)
    assert g.stats["nbtiles"] > 0
    g.set_grad_adjoint(gbar)
    g.gradients_adjoint()
    v = g.get_var_adjoint()
    g.close()
    check(v, p.fpoint, p.fnormal, p.pvolume, gbar, p.nown, what="boundary + interior groups")


@pytest.mark.parametrize("G", [2, 3, 4])
def test_adjoint_in_process_ranks(gpu, G):
    """G merged partitions on this GPU.  with_exchange: the whole mesh's adjoint on every owned point (global ids);
    without: every partition's own transpose"""
    pkg = gpu
    from cfd_proxy_amd import multigpu as mg
    dims, nd = (24, 20, 18), 12
    gp = pkg.gen_params(*dims, ndomains=nd)
    whole = pkg.gen_domain(pkg.gen_params(*dims, ndomains=1), 0)
    rng = np.random.default_rng(G)
    gbar_w = rng.standard_normal((whole.nall, 7, 3))
    ref_w = np_gradients_adjoint(whole.fpoint, whole.fnormal, whole.pvolume, gbar_w, whole.nown)
    scale_w = np.maximum(np.abs(ref_w), np_adjoint_scale(whole.fpoint, whole.fnormal, whole.pvolume, gbar_w, whole.nown))
    parts = [mg.build_rank_partition(gp, nd, G, r, via_files=False)[0] for r in range(G)]
    pkg.merge_link_group(parts)
    gids = []
    for r, p in enumerate(parts):  # global id of every merged point: merge_scatter of the merged index, per local domain
        gid = np.zeros(p.nall, np.int64)
        for dl, dd in enumerate(pkg.rank_domain_list(r, nd, G)):
            dom = pkg.gen_domain(gp, dd)
            merged = pkg.merge_scatter(p, dl, dom.nall, np.arange(p.nall, dtype=np.float64)[:, None])[:, 0].astype(np.int64)
            gid[merged] = pkg.gen_global_ids(gp, dd, dom.nall)
            dom.free()
        gids.append(gid)
    gparts = [pkg.GpuPartition(p, tile_points=64) for p in parts]
    for p, gq, gid in zip(parts, gparts, gids):
        gq.set_grad_adjoint(gbar_w[gid])
    for with_exchange in (True, False, True):
        pkg.group_adjoint(gparts, with_exchange)
        for p, gq, gid in zip(parts, gparts, gids):
            v = gq.get_var_adjoint()[: p.nown]
            if with_exchange:
                assert (np.abs(v - ref_w[gid[: p.nown]]) / scale_w[gid[: p.nown]]).max() <= TOL
            else:
                check(v, p.fpoint, p.fnormal, p.pvolume, gbar_w[gid], p.nown, strict=False, what=f"G={G} own")
    for gq in gparts:
        gq.close()
    whole.free()


def test_adjoint_rccl_self_exchange(gpu):
    """the RCCL form on one GPU: rank 0 of a 2-rank decomposition exchanges with ITSELF (as
    test_rccl_exchange_from_c_library_self_sendrecv does for the gradient): its ghost rows receive its own send rows, and
    the result is the adjoint with those rows (and their volumes) as ghost s"""
    pkg = gpu
    from cfd_proxy_amd import multigpu as mg
    gp = pkg.gen_params(12, 10, 8, ndomains=2)
    parts = [mg.build_rank_partition(gp, 2, 2, r, via_files=False)[0] for r in range(2)]
    reqs = [{int(k): (v[0], v[1]) for k, v in pkg.merge_requests(p).items()} for p in parts]
    for r, p in enumerate(parts):
        mg.exchange_requests(p, r, 2, None, all_requests=reqs)
    part = parts[0]
    si, ri = part.sendindex(1), part.recvindex(1)
    assert len(si) == len(ri) > 0
    rng = np.random.default_rng(4)
    gbar = rng.standard_normal((part.nall, 7, 3))
    g = pkg.GpuPartition(part, tile_points=32)
    lib = mg.RankSolver.torch_rccl_path()
    g.rccl_init(pkg.GpuPartition.rccl_unique_id(lib), 1, 0, rank_of_partner=[0], libpath=lib, self_exchange=True)
    g.set_grad_adjoint(gbar)
    g.step_adjoint_rccl(True)
    v = g.get_var_adjoint()
    g.step_adjoint_rccl(False)
    v0 = g.get_var_adjoint()
    g.close()
    gb, vol = gbar.copy(), part.pvolume.copy()
    gb[ri], vol[ri] = gbar[si], part.pvolume[si]
    check(v, part.fpoint, part.fnormal, vol, gb, part.nown, ghosts=True, strict=False, what="rccl self exchange")
    check(v0, part.fpoint, part.fnormal, part.pvolume, gbar, part.nown, strict=False, what="rccl, no exchange")


def test_adjoint_refused_with_ipc_transport(gpu):
    """a context whose xGMI write + notify transport is on: the group and step calls refuse on the host, before anything
    is enqueued"""
    pkg = gpu
    from cfd_proxy_amd import multigpu as mg
    gp = pkg.gen_params(12, 10, 8, ndomains=2)
    parts = [mg.build_rank_partition(gp, 2, 2, r, via_files=False)[0] for r in range(2)]
    reqs = [{int(k): (v[0], v[1]) for k, v in pkg.merge_requests(p).items()} for p in parts]
    mg.exchange_requests(parts[0], 0, 2, None, all_requests=reqs)
    g = pkg.GpuPartition(parts[0], tile_points=32)
    g.ipc_export()
    for s in range(len(g.partners())):
        g._ck(g.lib.cfdp_gpu_ipc_connect_loopback(g.h, s))
    g.ipc_ready()
    with pytest.raises(pkg.GpuError, match="write \\+ notify"):
        pkg.group_adjoint([g], True)
    with pytest.raises(pkg.GpuError, match="write \\+ notify"):
        g.step_adjoint_rccl(True)
    g.ipc_enable(False)
    g.close()


def test_adjoint_full_size(gpu):
    """the 64^3 lattice and the 262 k-point irregular stand-in against numpy"""
    pkg = gpu
    for conn in (None, pkg.CONN_IRREGULAR):
        kw = {} if conn is None else dict(connectivity=conn, numbering=1)
        dom = pkg.gen_domain(pkg.gen_params(64, 64, 64, ndomains=1, **kw), 0)
        fp, fn, vol, nown = dom.fpoint.copy(), dom.fnormal.copy(), dom.pvolume.copy(), dom.nown
        gbar = np.random.default_rng(64).standard_normal((dom.nall, 7, 3))
        v = run_adjoint(pkg, dom, gbar)
        dom.free()
        check(v, fp, fn, vol, gbar, nown, what=f"64^3 {'irregular' if conn else 'lattice'}")


def test_torch_op_gradcheck_and_backward(gpu):
    import torch
    pkg = gpu
    from cfd_proxy_amd.autograd import green_gauss
    dom = pkg.gen_domain(pkg.gen_params(4, 4, 4, ndomains=1), 0)
    part = pkg.GpuPartition(dom, tile_points=16)
    var = torch.randn(dom.nall, 7, dtype=torch.float64, device="cuda", requires_grad=True)
    # (the op is linear: the finite differences are exact up to rounding, |f| 2^-53 / eps ~ 1e-9 on this mesh's |grad| ~ 10)
    assert torch.autograd.gradcheck(lambda x: green_gauss(x, part), (var,), eps=1e-6, atol=1e-7, rtol=1e-7)
    part.close()
    dom.free()
    # forward == the ABI's gradient, backward == the ABI's adjoint, bit for bit, on a 20 x 18 x 16 mesh
    dom = pkg.gen_domain(pkg.gen_params(20, 18, 16, ndomains=1), 0)
    rng = np.random.default_rng(9)
    v_np = rng.standard_normal((dom.nall, 7))
    gbar = rng.standard_normal((dom.nall, 7, 3))
    part = pkg.GpuPartition(dom, tile_points=64)
    var = torch.tensor(v_np, device="cuda", requires_grad=True)
    out = green_gauss(var, part)
    out.backward(torch.tensor(gbar, device="cuda"))
    torch.cuda.synchronize()
    dom.var[:] = v_np
    part.push_fields()
    part.gradients()
    part.pull_fields()
    part.set_grad_adjoint(gbar)
    part.gradients_adjoint()
    vb = part.get_var_adjoint()
    assert np.array_equal(out.detach().cpu().numpy(), dom.grad)
    assert np.array_equal(var.grad.cpu().numpy(), vb)
    part.close()
    dom.free()


def test_adjoint_error_paths(gpu):
    import ctypes as C
    pkg = gpu
    lib = pkg.hip_lib()
    h = C.c_void_p()
    assert lib.cfdp_gpu_create(0, C.byref(h)) == 0
    buf = np.zeros(21)
    for rc in (lib.cfdp_gpu_set_grad_adjoint(h, buf.ctypes.data_as(C.POINTER(C.c_double))),
               lib.cfdp_gpu_get_var_adjoint(h, buf.ctypes.data_as(C.POINTER(C.c_double))),
               lib.cfdp_gpu_gradients_adjoint(h, None), lib.cfdp_gpu_step_adjoint_rccl(h, 0)):
        assert rc != 0 and b"no plan uploaded" in lib.cfdp_gpu_last_error()
    lib.cfdp_gpu_destroy(h)
    assert lib.cfdp_gpu_gradients_adjoint(None, None) != 0
    assert lib.cfdp_gpu_adjoint_group(None, 1, 1) != 0
    dom = pkg.gen_domain(pkg.gen_params(6, 6, 6, ndomains=1), 0)
    part = pkg.GpuPartition(dom)
    assert lib.cfdp_gpu_set_grad_adjoint(part.h, None) != 0 and b"null" in lib.cfdp_gpu_last_error()
    assert lib.cfdp_gpu_get_var_adjoint(part.h, None) != 0
    assert lib.cfdp_gpu_adjoint_ptrs(part.h, None, None) != 0
    # before any gbar was set: vbar is 0
    part.gradients_adjoint()
    assert not part.get_var_adjoint().any()
    part.close()
    dom.free()
