"""Multi-GPU plumbing of the scan path: one process per GPU (torch.distributed; backend
"nccl" is RCCL on ROCm, "gloo" on CPU for tests).  The DP itself needs no collective:
profiles are split into contiguous partitions (c-core/partition_size.c:13-16) or reads are
sharded, and only product rows / hit records are gathered at the end, in rank order -- which
is the reference's partition order (c-core/product.c:63-81)."""
from __future__ import annotations

import os


def env_rank():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(
        os.environ.get("WORLD_SIZE", "1"))


def partition_bounds(nelems: int, nparts: int):
    """[(first, count)] of every partition: ceil((N - i) / k) elements each, contiguous."""
    out, first = [], 0
    for i in range(nparts):
        size = (max(0, nelems - i) + nparts - 1) // nparts
        out.append((first, size))
        first += size
    return out


def shard(items, rank: int, world: int):
    """Contiguous shard `rank` of `items` with the same partition rule."""
    first, count = partition_bounds(len(items), world)[rank]
    return items[first : first + count]


def init_process_group(device=None):
    """Initialises torch.distributed from the torchrun environment (no-op for one process)."""
    import torch
    import torch.distributed as dist

    rank, local_rank, world = env_rank()
    if world <= 1 or dist.is_initialized():
        return rank, local_rank, world
    # DECIPHON_DIST_BACKEND=gloo: rehearsal of a multi-rank job on a box with fewer GPUs than ranks
    backend = os.environ.get("DECIPHON_DIST_BACKEND")
    if device is not None and str(device).startswith("cuda") and backend != "gloo":
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group("gloo")
    return rank, local_rank, world


def _all_gather_blobs(blob: bytes, count: int, device="cpu"):
    """[(bytes, count)] of every rank, in rank order, on every rank.  Two collectives: all_gather of the byte counts,
    then all_gather of the padded byte tensors."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    n = torch.tensor([len(blob), count], dtype=torch.int64, device=device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    cap = max(1, max(int(s[0]) for s in sizes))
    buf = torch.zeros(cap, dtype=torch.uint8, device=device)
    if blob:
        buf[: len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    bufs = [torch.zeros_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf)
    return [(bytes(b[: int(s[0])].cpu().numpy()), int(s[1])) for s, b in zip(sizes, bufs)]


def _one_process():
    import torch.distributed as dist

    return not dist.is_available() or not dist.is_initialized() or dist.get_world_size() == 1


def gather_rows(rows, device="cpu"):
    """All ranks' product rows, concatenated in rank order, on every rank."""
    if _one_process():
        return list(rows)
    out = []
    for blob, nrows in _all_gather_blobs(("\n".join(rows)).encode(), len(rows), device):
        if nrows:
            out += blob.decode().split("\n")
    return out


def gather_shards(rows, profiles, device="cpu"):
    """(rows_by_rank, profiles_by_rank) on every rank: each rank's product rows and, beside them, the database index of
    every row's profile -- what merge_read_shards takes."""
    import numpy as np

    profiles = np.ascontiguousarray(profiles, np.int32)
    if len(profiles) != len(rows):
        raise ValueError("one profile index per row")
    if _one_process():
        return [list(rows)], [profiles]
    rows_by_rank = [blob.decode().split("\n") if n else []
                    for blob, n in _all_gather_blobs(("\n".join(rows)).encode(), len(rows), device)]
    profiles_by_rank = [np.frombuffer(blob, np.int32, n).copy()
                        for blob, n in _all_gather_blobs(profiles.tobytes(), len(profiles), device)]
    return rows_by_rank, profiles_by_rank


def merge_read_shards(rows_by_rank, profiles_by_rank):
    """The rows of a scan whose reads were sharded over the ranks (shard(): contiguous, in batch order), in the whole
    scan's order.  Every rank's rows are in (profile, read, strand, window) order over its own reads, so the whole
    scan's order is: profile by profile and, within a profile, in rank order.  profiles_by_rank[r][i] is the database
    index of the profile of rows_by_rank[r][i] (non-decreasing along i).  A pure function: no process group is asked."""
    keyed = []
    for rank, (rows, profiles) in enumerate(zip(rows_by_rank, profiles_by_rank)):
        if len(rows) != len(profiles):
            raise ValueError(f"rank {rank}: {len(rows)} rows, {len(profiles)} profile indices")
        keyed += [(int(p), rank, i) for i, p in enumerate(profiles)]
    keyed.sort()
    return [rows_by_rank[rank][i] for _, rank, i in keyed]


PRODUCTS_HEADER = "sequence\twindow\twindow_start\twindow_stop\thit\thit_start\thit_stop\tprofile\tabc\tlrt\tevalue\tmatch"


def products_header(strands="plus") -> str:
    """The header line DcpProductRuns writes (csrc/product_runs.cpp), without its newline: 12 columns, 13 on both strands."""
    from .hip import strands_code

    return PRODUCTS_HEADER + ("\tstrand" if strands_code(strands) == 1 else "")


def scan_partitioned(dbfile, sequences, product_dir, multi_hits: bool = True, hmmer3_compat: bool = False,
                     backend: str | None = None, balanced: bool = True, strands="plus", calibrate=None,
                     evalue_z: float = 0.0, evalue_max: float = float("inf")):
    """One scan over all GPUs of the job (run under torchrun, one process per GPU): rank i scans the
    i-th contiguous profile partition (c-core/partition_size.c:13-16 -- what thread i of
    c-core/scan.c:188-208 would take) against all the reads; the product rows are gathered in
    rank order, which is the reference's row order (c-core/product.c:63-81), and rank 0 writes
    product_dir/products.tsv.  sequences: [(id, name, text)].  Returns all rows on every rank.
    balanced (default): the partition boundaries balance the sum of core sizes -- DP cells go with K -- instead
    of the number of profiles; contiguous and in order either way, so the row order is the same.

    backend: "nccl" (RCCL; the default when every rank has its own GPU) or "gloo" (also lets several
    ranks share one GPU, as the tests on a one-GPU box do).

    What a scan takes: strands="both" (the header gains the strand column); calibrate= a dict of the arguments of
    Scan.calibrate_lengths, or of Scan.calibrate when it has "length" -- each rank calibrates the profiles it owns, and
    the random reads are a function of the seed alone; evalue_z and evalue_max as Scan.set_evalue.  Every rank sees all
    reads, so the default Z, the sequences a run scans, is the same everywhere.

    Failures: a setup, calibration or run that raises does so before this rank reaches the gather, and the other ranks
    then wait in it until the launcher ends the job (torchrun does, once one rank has exited with an error)."""
    import torch
    import torch.distributed as dist

    from .scan import Batch, Scan, Sequence

    rank, local_rank, world = env_rank()
    ndev = max(1, torch.cuda.device_count())
    backend = backend or os.environ.get("DECIPHON_DIST_BACKEND") or ("nccl" if ndev >= world else "gloo")
    device = local_rank % ndev
    if world > 1 and not dist.is_initialized():
        if backend == "nccl":
            torch.cuda.set_device(device)
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group("gloo")
    batch = Batch()
    for sid, name, text in sequences:
        batch.add(Sequence(sid, name, text))
    part_dir = os.path.join(str(product_dir), f"part{rank}")
    with Scan(dbfile, 0, 1, multi_hits, hmmer3_compat, False, partition=(device, rank, world), balanced=balanced,
              strands=strands) as scan:
        if calibrate is not None:
            (scan.calibrate if "length" in calibrate else scan.calibrate_lengths)(**calibrate)
        scan.set_evalue(evalue_z, evalue_max)
        scan.run(part_dir, batch)
        rows = scan.products()
    rows = gather_rows(rows, f"cuda:{device}" if backend == "nccl" and world > 1 else "cpu")
    if rank == 0:
        with open(os.path.join(str(product_dir), "products.tsv"), "w") as f:
            f.write(products_header(strands) + "\n")
            for r in rows:
                f.write(r + "\n")
    if world > 1:
        dist.barrier()
    return rows
