"""CPU, world_size 2 over gloo: the check every sharded run makes before its first step (SVIRunner._assert_same_tuning_on_every_rank,
a MIN and a MAX all-reduce of a digest of Tuning, layout, exchange size and likelihood kernel).  The count storage of a rank (uint16
when every count of ITS shard is an integer <= 65535, float32 otherwise) shows in the kernel name as `,u16` and is the same arithmetic
on the same layout: ranks that differ in it only must pass.  Ranks that differ in genes per lane or in the exchange size must not."""
import os
import sys
import types

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KERNEL = "vc_main_kernel<1,1,vfull_nb,gpl{gpl}{u16},pwl>"


class _StandInEngine:
    """The part of HipEngine the digest reads."""

    def __init__(self, rank, main_kernel, xsize, header=4, n_global=1234, onehot=0):
        import torch
        self.rank, self.header, self.n_global, self._x = rank, header, n_global, xsize
        self.device = torch.device("cpu")
        self.stats = {"main_kernel": main_kernel, "onehot_batches": onehot, "count_storage": "u16" if ",u16" in main_kernel else "f32"}

    def exchange_size(self):
        return self._x


def _worker(rank, world, port, per_rank, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from velocycle_amd.svi import SVIRunner
    from velocycle_amd.tuning import Tuning
    kernel, xsize = per_rank[rank]
    me = types.SimpleNamespace(e=_StandInEngine(rank, kernel, xsize), tuning=Tuning(), pg=None)
    try:
        SVIRunner._assert_same_tuning_on_every_rank(me)
        q.put((rank, "ok"))
    except Exception as ex:                      # noqa: BLE001 -- reported to the parent
        q.put((rank, f"{type(ex).__name__}: {ex}"))
    dist.barrier()
    dist.destroy_process_group()


def _run(per_rank):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, world, port, per_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [res[r] for r in range(world)]


def test_kernel_layout_name_drops_only_the_storage_tag():
    from velocycle_amd.svi import kernel_layout_name
    assert kernel_layout_name("vc_main_kernel<1,1,vfull_nb,gpl8,u16,pwl>") == "vc_main_kernel<1,1,vfull_nb,gpl8,pwl>"
    assert kernel_layout_name("vc_main_kernel<1,2,phase_nb,gpl4,u16>") == "vc_main_kernel<1,2,phase_nb,gpl4>"
    assert kernel_layout_name("vc_main_kernel<1,2,phase_nb,gpl4>") == "vc_main_kernel<1,2,phase_nb,gpl4>"
    assert kernel_layout_name("vc_main_kernel<1,1,vu_nb,gpl8,pwl>") == "vc_main_kernel<1,1,vu_nb,gpl8,pwl>"


@pytest.mark.parametrize("tags", [("", ",u16"), (",u16", ""), (",u16", ",u16"), ("", "")])
def test_ranks_that_differ_only_in_count_storage_pass(tags):
    """One shard holds a count > 65535 (or a non-integer one) and stores float32, the other uint16: one sharded run."""
    per_rank = [(KERNEL.format(gpl=8, u16=t), 5000) for t in tags]
    assert _run(per_rank) == ["ok", "ok"]


@pytest.mark.parametrize("case", ["genes_per_lane", "exchange_size", "genes_per_lane_and_storage"])
def test_ranks_that_differ_in_layout_are_refused(case):
    per_rank = {"genes_per_lane": [(KERNEL.format(gpl=8, u16=""), 5000), (KERNEL.format(gpl=4, u16=""), 5000)],
                "exchange_size": [(KERNEL.format(gpl=8, u16=",u16"), 5000), (KERNEL.format(gpl=8, u16=",u16"), 5064)],
                "genes_per_lane_and_storage": [(KERNEL.format(gpl=8, u16=",u16"), 5000), (KERNEL.format(gpl=4, u16=""), 5000)]}[case]
    res = _run(per_rank)
    for r, msg in enumerate(res):
        assert msg.startswith("HipEngineError") and "do not share one Tuning / layout" in msg, (r, msg)
