"""GPU: deciphon_amd.dist.scan_partitioned with what a scan takes -- both strands, a calibration over a ladder of read
lengths, an E-value limit -- in one process and with two ranks under torchrun."""
import os
import socket
import subprocess
import sys

import pytest

from dcp_testlib import GOLDEN, ROOT, read_fasta

pytestmark = pytest.mark.gpu

DCP = os.path.join(GOLDEN, "minifam.dcp")
LADDER = dict(nseq=40, lengths=(90, 300), lam=0)


def minifam_reads():
    both = read_fasta(os.path.join(GOLDEN, "consensus.fna")) + read_fasta(os.path.join(GOLDEN, "consensus_multi.fna"))
    return [(i, f"seq{i}", text) for i, (_, text) in enumerate(both)]


def evalue_limit(rows):
    """A limit between two E-values of `rows`, where their relative gap is largest: some rows stay, some go."""
    v = sorted({float(r.split("\t")[10]) for r in rows})
    assert len(v) >= 2, v
    k = max(range(1, len(v)), key=lambda i: (v[i] - v[i - 1]) / v[i])
    return (v[k - 1] + v[k]) / 2


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """The single-GPU scan: both strands, calibrated; (limit, products.tsv under the limit)."""
    from deciphon_amd.scan import Batch, Scan, Sequence

    d = tmp_path_factory.mktemp("single")
    batch = Batch()
    for sid, name, text in minifam_reads():
        batch.add(Sequence(sid, name, text))
    with Scan(DCP, 0, 1, True, False, False, strands="both") as scan:
        scan.calibrate_lengths(**LADDER)
        scan.run(str(d / "all"), batch)
        unfiltered = scan.products()
        limit = evalue_limit(unfiltered)
        scan.set_evalue(max=limit)
        scan.run(str(d / "limited"), batch)
        assert 0 < len(scan.products()) < len(unfiltered)  # at least one row kept, at least one dropped
    return limit, (d / "limited" / "products.tsv").read_text()


def test_one_process_takes_strands_calibration_and_the_limit(tmp_path, single):
    from deciphon_amd import dist as ddist

    limit, want = single
    rows = ddist.scan_partitioned(DCP, minifam_reads(), str(tmp_path), strands="both", calibrate=LADDER, evalue_max=limit)
    got = (tmp_path / "products.tsv").read_text()
    assert got == want and got.splitlines()[0].endswith("\tstrand") and got.splitlines()[1:] == rows


def test_two_ranks_take_strands_calibration_and_the_limit(tmp_path, single):
    """scripts/scan_multi_gpu.py under torchrun with 2 ranks (both on this box's one GPU, rows gathered over gloo):
    products.tsv is the single-process scan's, header and all."""
    limit, want = single
    fasta = tmp_path / "reads.fna"
    fasta.write_text("".join(f">{name}\n{text}\n" for _, name, text in minifam_reads()))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DECIPHON_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "scripts", "scan_multi_gpu.py"), "--strands", "both", "--calibrate", "90,300",
                        "--nseq", "40", "--lam", "0", "--evalue-max", repr(limit), DCP, str(fasta), str(tmp_path / "multi")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "multi" / "products.tsv").read_text() == want
