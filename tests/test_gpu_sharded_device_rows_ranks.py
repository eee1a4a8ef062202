"""impg_gpu_query_batch_device in rank processes (torch.distributed.run, one process per rank): collective calls over
the host transport (ranks share GPU 0) and RCCL, worker tests/device_rows_rank_worker.py."""
import os
import subprocess
import sys

import pytest

from tests.test_multi_gpu import write_paf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_rows_ranks(world, args, port, lanes=2, timeout=900):
    """run_ranks (tests/test_multi_cpu.py) with this file's worker"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", IMPG_TEST_LANES=str(lanes))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "tests", "device_rows_rank_worker.py")] + args,
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("world,lanes", [(2, 2), (3, 1)])
def test_rank_device_rows_host_transport(tmp_path, world, lanes):
    path = write_paf(tmp_path)
    out = run_rows_ranks(world, ["host", path], 29780 + world, lanes=lanes)
    assert "device rows ok world=%d lanes=%d transport=host" % (world, lanes) in out


def test_rank_device_rows_rccl(tmp_path):
    path = write_paf(tmp_path)
    out = run_rows_ranks(1, ["rccl", path], 29790, lanes=2)
    assert "device rows ok world=1 lanes=2 transport=rccl" in out
