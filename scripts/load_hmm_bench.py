#!/usr/bin/env python3
"""From a HMMER3 file to a scan that is set up, two ways, on the Pfam-shaped synthetic file of press_bench.py:

  (a) the route through a file: dcp_press_* to a .dcp, then dcp_scan_setup on it (page cache warm: just written);
  (b) the direct route: dcp_scan_setup_hmm, with the phase seconds dcp_hip_load_hmm prints under DECIPHON_HIP_TIMING;
  (c) the rows kernel alone, from (b)'s HIP-event seconds: pool bytes written per second, beside a device-to-device
      copy of as many bytes (hipMemcpyAsync, HIP events) -- the yardstick for a kernel that only moves data.

  (d) --set-epsilon, instead of the routes: a full Engine.load_hmm, then Engine.set_epsilon on that engine -- wall clock
      of both, the load's emission + rows kernel seconds beside the one re-emission kernel's, which does their work.

The routes alternate, --runs times each.  Prints a line per run and one JSON line.  `--route direct --runs 1` is what
to put behind `rocprofv3 --kernel-trace --stats --` for the kernels' shares of the load."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deciphon_amd import Press, synth  # noqa: E402
from deciphon_amd.scan import Scan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--profiles", type=int, default=2000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--epsilon", type=float, default=0.01)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--route", choices=["both", "file", "direct"], default="both")
ap.add_argument("--dir", default=None, help="where the .hmm and .dcp go (default: a temporary directory)")
ap.add_argument("--set-epsilon", action="store_true",
                help="instead of the routes: --runs times a full Engine.load_hmm, then Engine.set_epsilon on that "
                     "engine (to --to-epsilon), wall clock and kernel seconds of both")
ap.add_argument("--to-epsilon", type=float, default=0.1)
args = ap.parse_args()

work = args.dir or tempfile.mkdtemp(prefix="load_hmm_bench_")
os.makedirs(work, exist_ok=True)
hmm, dcp = os.path.join(work, "pfam_like.hmm"), os.path.join(work, "pfam_like.dcp")
seeds = synth.load_hmm_seeds(os.path.join(ROOT, "tests", "golden", "minifam.hmm"))
nprof = synth.write_hmm(hmm, synth.pfam_like_hmms(seeds, args.profiles, args.seed))

TIMING = re.compile(r"dcp_hip_load_hmm: (\d+) profiles, ([\d.]+) GB of tables; parse ([\d.]+) s, upload ([\d.]+) s, "
                    r"emission kernel ([\d.]+) s, rows kernel ([\d.]+) s, wait ([\d.]+) s")


def stderr_of(call):
    """Runs call() with the process's stderr (the library writes to it) going to a file; -> (result, text)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def file_route():
    t0 = time.perf_counter()
    with Press(hmm, dcp, 1, args.epsilon) as p:
        while not p.end():
            p.next()
    t_press = time.perf_counter() - t0
    size = os.path.getsize(dcp)
    t0 = time.perf_counter()
    scan = Scan(dcp, 0, 1, True, False, False)
    t_setup = time.perf_counter() - t0
    scan.free()
    os.unlink(dcp)
    return dict(press_s=t_press, setup_warm_s=t_setup, total_s=t_press + t_setup, dcp_gb=size / 1e9)


def direct_route():
    os.environ["DECIPHON_HIP_TIMING"] = "1"
    t0 = time.perf_counter()
    scan, text = stderr_of(lambda: Scan.from_hmm(hmm, 1, args.epsilon))
    t_total = time.perf_counter() - t0
    del os.environ["DECIPHON_HIP_TIMING"]
    scan.free()
    m = TIMING.search(text)
    assert m, text
    v = [float(x) for x in m.groups()]
    return dict(total_s=t_total, profiles=int(v[0]), pool_gb=v[1], parse_s=v[2], upload_s=v[3], emission_kernel_s=v[4],
                rows_kernel_s=v[5], wait_s=v[6], rows_gb_per_s=v[1] / v[5] if v[5] else None)


def device_copy_gb_per_s(nbytes):
    """hipMemcpy device to device of nbytes, timed with HIP events; the best of three."""
    import ctypes as C

    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    nbytes = int(nbytes)

    def ok(rc):
        assert rc == 0, rc

    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes)))
    ok(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)))
    ok(hip.hipMemset(a, 0, C.c_size_t(nbytes)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    best = 0.0
    for i in range(4):  # the first one warms
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, None))  # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float(0)
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i:
            best = max(best, nbytes / 1e9 / (ms.value * 1e-3))
    for ev in (e0, e1):
        ok(hip.hipEventDestroy(ev))
    for p in (a, b):
        ok(hip.hipFree(p))
    return best


RETIMING = re.compile(r"dcp_hip_set_epsilon: (\d+) profiles, (\d+) nodes, (\d+) bytes written; re-emission kernel ([\d.]+) s")


def set_epsilon_leg():
    """A full load, then a change of the error rate on the same engine: the load's emission + rows kernels do the work
    of the one re-emission kernel, through the scratch buffer."""
    from deciphon_amd import Engine

    os.environ["DECIPHON_HIP_TIMING"] = "1"
    with Engine(0) as eng:
        t0 = time.perf_counter()
        _, text = stderr_of(lambda: eng.load_hmm(hmm, 1, args.epsilon))
        t_load = time.perf_counter() - t0
        m = TIMING.search(text)
        assert m, text
        v = [float(x) for x in m.groups()]
        t0 = time.perf_counter()
        _, text = stderr_of(lambda: eng.set_epsilon(args.to_epsilon))
        t_set = time.perf_counter() - t0
        m = RETIMING.search(text)
        assert m, text
        w = m.groups()
        out = dict(load_s=t_load, emission_kernel_s=v[4], rows_kernel_s=v[5], load_kernels_s=v[4] + v[5],
                   set_epsilon_s=t_set, reemit_kernel_s=float(w[3]), nodes=int(w[1]), bytes_written=int(w[2]),
                   written_gb_per_s=int(w[2]) / 1e9 / float(w[3]) if float(w[3]) else None,
                   pool_bytes=eng.pool_bytes, dist_bytes=eng.dist_bytes)
    del os.environ["DECIPHON_HIP_TIMING"]
    return out


res = dict(profiles=nprof, hmm_mb=os.path.getsize(hmm) / 1e6, epsilon=args.epsilon, file=[], direct=[])
if args.set_epsilon:
    res["to_epsilon"], res["set_epsilon"] = args.to_epsilon, []
    for run in range(args.runs):
        r = set_epsilon_leg()
        res["set_epsilon"].append(r)
        print(f"run {run} load: {r['load_s']:.3f} s, emission kernel {r['emission_kernel_s']:.4f} + rows kernel "
              f"{r['rows_kernel_s']:.4f} = {r['load_kernels_s']:.4f} s | set_epsilon: {r['set_epsilon_s']:.4f} s, "
              f"re-emission kernel {r['reemit_kernel_s']:.4f} s, {r['written_gb_per_s']:.0f} GB/s written; "
              f"distributions {r['dist_bytes'] / 1e6:.1f} MB beside a pool of {r['pool_bytes'] / 1e6:.1f} MB", flush=True)
    args.runs = 0
for run in range(args.runs):
    if args.route in ("both", "file"):
        r = file_route()
        res["file"].append(r)
        print(f"run {run} (a) file:   press {r['press_s']:.3f} s + setup {r['setup_warm_s']:.3f} s = {r['total_s']:.3f} s "
              f"({r['dcp_gb']:.2f} GB .dcp)", flush=True)
    if args.route in ("both", "direct"):
        r = direct_route()
        res["direct"].append(r)
        print(f"run {run} (b) direct: {r['total_s']:.3f} s; parse {r['parse_s']:.3f}, upload {r['upload_s']:.3f}, emission "
              f"kernel {r['emission_kernel_s']:.4f}, rows kernel {r['rows_kernel_s']:.4f}, wait {r['wait_s']:.3f} s; "
              f"{r['pool_gb']:.2f} GB of pool, rows kernel {r['rows_gb_per_s']:.0f} GB/s written", flush=True)
if res["direct"]:
    res["device_copy_gb_per_s"] = device_copy_gb_per_s(res["direct"][0]["pool_gb"] * 1e9)
    print(f"(c) device-to-device copy of as many bytes: {res['device_copy_gb_per_s']:.0f} GB/s written", flush=True)
print(json.dumps(res))
os.unlink(hmm)
if not args.dir:
    os.rmdir(work)
