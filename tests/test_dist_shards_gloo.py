"""CPU, world_size 2 over gloo: the exchange of a scan whose reads are sharded -- every rank's rows and, beside them, the
profile index of every row are gathered, and merged into the whole scan's order (deciphon_amd.dist.gather_shards,
merge_read_shards)."""
import os
import socket
import subprocess
import sys
import textwrap

from dcp_testlib import ROOT

WORKER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, {root!r})
    import numpy as np
    import torch.distributed as dist
    from deciphon_amd import dist as ddist
    rank, local_rank, world = ddist.init_process_group("cpu")
    assert world == 2 and dist.get_backend() == "gloo"
    # the whole scan: (profile, read) rows in that order; reads 0..4, sharded contiguously: rank 0 has 0..2, rank 1 has 3, 4
    reads = list(range(5))
    hits = [(0, 0), (0, 1), (0, 3), (1, 4), (2, 2), (2, 3), (2, 4), (4, 1)]
    whole = ["PF%05d\\tread%d" % h for h in hits]
    mine = set(ddist.shard(reads, rank, world))
    assert mine == ({{0, 1, 2}} if rank == 0 else {{3, 4}})
    own = [h for h in hits if h[1] in mine]
    rows = ["PF%05d\\tread%d" % h for h in own]
    rows_by_rank, profiles_by_rank = ddist.gather_shards(rows, np.array([p for p, _ in own], np.int32), "cpu")
    assert len(rows_by_rank) == 2 and rows_by_rank[rank] == rows
    assert [p.tolist() for p in profiles_by_rank] == [[0, 0, 2, 4], [0, 1, 2, 2]]
    assert all(p.dtype == np.int32 for p in profiles_by_rank)
    assert ddist.merge_read_shards(rows_by_rank, profiles_by_rank) == whole
    # a rank without rows, then no rows at all
    r2, p2 = ddist.gather_shards(rows if rank == 1 else [], [p for p, _ in own] if rank == 1 else [], "cpu")
    assert r2[0] == [] and len(p2[0]) == 0
    assert ddist.merge_read_shards(r2, p2) == [w for w, h in zip(whole, hits) if h[1] in (3, 4)]
    r3, p3 = ddist.gather_shards([], [], "cpu")
    assert ddist.merge_read_shards(r3, p3) == []
    dist.barrier()
    dist.destroy_process_group()
    open(os.path.join({outdir!r}, "rank%d.ok" % rank), "w").write("ok")
""")


def test_two_ranks_gather_and_merge_read_shards(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, outdir=str(tmp_path)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(script)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists()
