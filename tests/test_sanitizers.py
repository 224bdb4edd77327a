"""Sanitizer builds of the C host side, on the CPU (the GPU pool offers none): AddressSanitizer + UBSan over the
loader / generator / merger / tiler, ThreadSanitizer over the call election."""
import os
import platform
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "cfd-proxy_amd")


def _gcc_lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def _without_aslr(cmd):
    """this gcc's ThreadSanitizer expects the program and its libraries inside fixed address ranges, which a kernel that
    randomises with more bits (vm.mmap_rnd_bits = 32) can place them outside of ("FATAL: ThreadSanitizer: unexpected
    memory mapping", before main()): the test host runs with address-space randomisation off for that one process
    (setarch -R sets a personality flag of the child; nothing system-wide changes)"""
    setarch = shutil.which("setarch")
    return [setarch, platform.machine(), "-R", *cmd] if setarch else list(cmd)


@pytest.mark.skipif(_gcc_lib("libtsan.so") is None, reason="no libtsan in this image")
@pytest.mark.parametrize("scenario,env,want", [
    ("team", {}, "performed 400 of 400"), ("serial_threads", {}, "performed 14 of 14"), ("mixed", {}, "performed 158 of 158"),
    ("master", {}, "performed 80 of 80"), ("pthread_team", {}, "performed 100 of 100"),
    ("team_then_master", {}, "performed 160 of 160"), ("single", {"CFDP_CALL_MODE": "every"}, "performed 80 of 80"),
    ("single", {}, None)])
def test_call_election_under_thread_sanitizer(pkg, scenario, env, want):
    """host/call_election.c built with -fsanitize=thread together with its test host: the reference's every-thread team
    (team mates running ahead of each other), serial callers on ever new threads, teams of 4 -> 2 -> 4 with serial calls
    in between (a shrinking and re-growing team), omp master, a declared pthread team, every-thread regions followed by
    master sections, omp single with and without CFDP_CALL_MODE=every (without: either nothing is lost or the run stops
    with the library's message -- never a sanitizer report).  Suppressed, top frame only: the test host's own outlined
    region bodies (libgomp's hand-over of a region's arguments is invisible to the sanitizer), nothing of the library"""
    r = subprocess.run(["make", "-C", PKG, "tsan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    e = {k: v for k, v in os.environ.items() if k != "CFDP_CALL_MODE"}
    e.update(env, TSAN_OPTIONS="halt_on_error=1 exitcode=66 suppressions=" + os.path.join(ROOT, "tests", "tsan.supp"))
    r = subprocess.run(_without_aslr([os.path.join(PKG, "build", "tsan", "host_call_election"), scenario]), capture_output=True,
                       text=True, timeout=300, env=e)
    assert "ThreadSanitizer" not in r.stderr and r.returncode != 66, r.stderr[-3000:]
    if want:
        assert r.returncode == 0 and want in r.stdout, r.stdout + r.stderr[-1500:]
    else:
        assert (r.returncode == 0 and "performed 80 of 80" in r.stdout) or \
            (r.returncode == 1 and "not by every thread of the team" in r.stderr), r.stdout + r.stderr[-1500:]


@pytest.mark.skipif(_gcc_lib("libasan.so") is None, reason="no libasan in this image")
def test_host_side_under_address_and_ub_sanitizer(pkg):
    """the C host side (NetCDF reader / writer, generator, loader, merger, tiler, communication tables, call election)
    built with -fsanitize=address,undefined; the host test files run against that build in a child interpreter"""
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pre = " ".join(x for x in (_gcc_lib("libasan.so"), _gcc_lib("libubsan.so")) if x)
    e = dict(os.environ, CFDP_LIBDIR=os.path.join(PKG, "build", "asan"), LD_PRELOAD=pre,
             ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_host_mesh.py"),
                        os.path.join(ROOT, "tests", "test_host_io.py"), "-x", "-q", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, timeout=900, env=e, cwd=ROOT)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert " passed" in r.stdout
