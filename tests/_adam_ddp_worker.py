"""One rank of tests/test_gpu_adam.py's DDP test (not collected by pytest): the tiny model of
tests/_ddp_worker.py, its half of the 2-clip batch, three Trainer steps with optimizer="hip",
skip_bad_steps=1 and clip_grad_norm=inf over gloo.  Rank 1's loss is NaN on the second step: the
averaged gradients, and so their norm, are non-finite on BOTH ranks, and both skip.

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_adam_ddp_worker.py OUT
Writes OUT.rank<r>.pt: {"initial": {name: tensor}, "params": [the same after each step],
"finite_loss", "skipped", "flags" (skip_flag), "lr": per step, "tripped_at",
"missing_clipper_error": Trainer refused skip_bad_steps without clip_grad_norm, "bucketed"}.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ddp_worker as w  # noqa: E402  (sets the import paths and the gloo backend)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from vdiff.ddp import broadcast_parameters, init_from_env  # noqa: E402


def _named(m):
    return {n: p.detach().cpu().clone() for n, p in m.named_parameters()}


def main(out):
    rank, world, local = init_from_env()          # gloo: no GPU call before this point
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    from vdiff import ops
    from vdiff.engine import Clip, Trainer
    from vdiff.schedulers import LinearNoiseScheduler
    m = w.build(dev)
    broadcast_parameters(m)
    sched = LinearNoiseScheduler(100, 0.00085, 0.012)
    try:
        Trainer(m, sched, lr=1e-3, bucket_mb=0.25, optimizer="hip", skip_bad_steps=1)
        refused = False
    except ValueError as e:
        refused = "clip_grad_norm" in str(e)
    assert all(p.grad is None for p in m.parameters())   # refused before any bucket was made
    calls = []

    def loss_fn(pred, eps):
        calls.append(1)
        loss = ops.mse_loss(pred, eps)
        return loss * float("nan") if rank == 1 and len(calls) == 2 else loss

    tr = Trainer(m, sched, lr=1e-3, bucket_mb=0.25, optimizer="hip", lr_warmup=2,
                 skip_bad_steps=1, clip_grad_norm=float("inf"), loss_fn=loss_fn, check_every=100)
    initial = _named(m)
    x0, cond, feat, eps, t = w.batch(dev)
    T = x0.shape[2]
    sl = slice(rank, rank + 1)
    clip = Clip(x0[sl], cond[sl], feat[rank * T:(rank + 1) * T], eps[sl], t[sl])
    rec = {"params": [], "finite_loss": [], "skipped": [], "flags": [], "lr": []}
    for _ in range(3):
        loss = tr.step(clip)
        rec["params"].append(_named(m))
        rec["finite_loss"].append(bool(torch.isfinite(loss)))
        rec["skipped"].append(int(tr.skipped_steps))
        rec["flags"].append(int(tr.opt.skip_flag))
        rec["lr"].append(float(tr.lr))
    tr.check_finite()
    rec.update(initial=initial, tripped_at=int(tr.opt.tripped_at), missing_clipper_error=refused,
               bucketed=tr.bucketer is not None)
    torch.save(rec, f"{out}.rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
