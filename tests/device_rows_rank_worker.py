"""Worker of tests/test_gpu_sharded_device_rows_ranks.py (one process per rank, launched by torch.distributed.run):
impg_gpu_query_batch_device in rank processes.  Every rank submits its own ranges (collective calls); check() is
collective; rank 0 gathers every rank's parts and checks the collective batch's rows against the oracle.

  <transport> <paf>   transport = host (gloo callbacks, ranks share GPU 0) or rccl (one GPU per rank)
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import impg_amd  # noqa: E402
from tests.multi_worker import make_comm  # noqa: E402


def main():
    transport, paf_path = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    lanes = int(os.environ.get("IMPG_TEST_LANES", "2"))
    from oracle import oracle as o
    from tests.paf_gen import random_ranges
    from tests.test_gpu_fullsize import checksum
    device = int(os.environ.get("LOCAL_RANK", "0")) if transport == "rccl" else 0
    comm = make_comm(transport, rank, world, lanes, device)
    c = o.OracleIndex(paf_paths=[paf_path], preparse=True)
    g = impg_amd.GpuImpg.from_paf(paf_path, device=device, comm=comm)
    g.set_option("chunk_ranges", 7)
    n_seq, seq_len = c.num_seqs(), int(c.seq_len(0))
    n_q = 0 if (rank == 1 and world > 1) else 11 + 6 * rank  # different counts per rank; one rank has none
    rl = random_ranges(300 + rank, n_q, n_seq, seq_len, max_len=3000, min_len=120)
    sizes = [None] * world
    dist.all_gather_object(sizes, n_q)
    offset, total = sum(sizes[:rank]), sum(sizes)
    all_rl = [None] * world
    dist.all_gather_object(all_rl, rl)
    batch = [r for part in all_rl for r in part]
    cases = [dict(), dict(transitive=True, max_depth=1, min_transitive_len=20),
             dict(transitive=True, max_depth=3, min_transitive_len=20, min_distance_between_ranges=0),
             dict(transitive=True, max_depth=0, min_transitive_len=30, min_output_length=60),
             dict(transitive=True, max_depth=3, min_identity=0.7)]
    d_ranges = torch.from_numpy(impg_amd.GpuImpg._ranges(rl).view(np.uint8)).to("cuda:%d" % device) if n_q else None
    for ci, kw in enumerate(cases):
        p = impg_amd.make_params(**kw)
        if ci == 2:  # ranges already in HBM (each rank's own pointer; a rank without ranges passes none)
            dr = g.query_batch_device(None, p, device_ptr=d_ranges.data_ptr() if n_q else 0, n=n_q)
        else:
            dr = g.query_batch_device(rl, p)
        assert dr.batch_offset() == (offset, total), (rank, dr.batch_offset(), offset, total)
        cnt, ck = dr.check()  # collective
        mo = kw.get("min_output_length") if kw.get("transitive") else None
        proj = 0
        for i, (t, s, e) in enumerate(rl):
            want = c.query(t, s, e, **kw)[1:]
            proj += c.last_projection_count()
            assert int(cnt[i]) == len(want) and int(ck[i]) == checksum(want), (rank, i, kw)
        tt = torch.tensor([dr.projected, proj], dtype=torch.int64)
        dist.all_reduce(tt)  # projections are counted where they are computed: compare the global sums
        assert int(tt[0]) == int(tt[1]), (rank, kw, tt.tolist())
        parts = [dr.part_to_host(k) for k in range(len(dr.parts()))]
        gathered = [None] * world
        dist.all_gather_object(gathered, parts)
        if rank == 0:
            rows = [[] for _ in range(total)]
            for rp in gathered:
                for first, level, qid, co, src, fr in rp:
                    live = qid != np.uint32(0xFFFFFFFF)
                    if mo is not None:
                        live &= np.abs(co[:, 1].astype(np.int64) - co[:, 0]) >= mo
                    assert (src < len(fr)).all()
                    f = fr[src[live]]
                    for q, r, tg in zip((first + f["range_idx"]).tolist(), np.column_stack([qid[live], co[live]]).tolist(), f["target_id"].tolist()):
                        rows[q].append((r[0], r[1], r[2], tg, r[3], r[4]))
            for i, (t, s, e) in enumerate(batch):
                want = sorted(tuple(int(x) for x in r) for r in c.query(t, s, e, **kw)[1:].tolist())
                assert sorted(rows[i]) == want, (kw, i)
        dr.free()
    dist.barrier()
    if rank == 0:
        print("device rows ok world=%d lanes=%d transport=%s" % (world, lanes, transport))
    del g
    comm.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
