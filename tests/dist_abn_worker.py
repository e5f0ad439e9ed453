#!/usr/bin/env python3
"""Worker of tests/test_abn.py::test_sync_variant_two_ranks_equal_one_process_on_the_whole_batch — launched with
`python -m torch.distributed.run --nproc-per-node 2`: InPlaceABNSync (cspn_monodepth_amd/network/inplace_abn.py) with every
rank on the one visible GPU (backend gloo) or one GPU each (nccl).  Reference behaviour being replaced: the thread-and-queue
rendezvous of network/libs/inplace_abn/functions.py:165-298.

Each rank takes its contiguous share of ONE seeded batch of 4 and runs forward + backward through InPlaceABNSync; every rank also
runs a plain InPlaceABN on the whole batch.  Asserted on every rank, at 1e-5 of the largest magnitude:
  * the rank's outputs and dx equal the whole batch's rows of that rank;
  * the parameter gradients SUMMED over the ranks equal the whole batch's (a rank's dweight / dbias are the global edz / eydz
    times its own N * S, as in the reference, whose DataParallel adds the replicas' gradients);
  * the running statistics equal the whole batch's — and are identical across the ranks bit for bit.
Two shapes: 4 x 6 x 9 x 11 (a rank's half is in the SMALL regime) and 4 x 3 x 40 x 61 (SPLIT), leaky_relu and elu."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BAR = 1e-5


def close(got, want, what):
    err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
    assert err <= BAR, (what, err)
    return err


def main():
    import abn_cases as ac
    from cspn_monodepth_amd.network import inplace_abn as A
    backend = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    worst = 0.0
    for k, (shape, act) in enumerate((((4, 6, 9, 11), "leaky_relu"), ((4, 3, 40, 61), "elu"))):
        per = shape[0] // world
        regime = A.abn_plan(per, shape[1], shape[2] * shape[3])["regime"]
        assert regime == ("small", "split")[k], regime
        case = ac._case(shape, act, 330 + k)
        inp = ac.make_inputs(case)
        t = {n: torch.from_numpy(v).to(dev) for n, v in inp.items()}

        def module(cls):
            m = cls(shape[1], activation=act).to(dev)
            with torch.no_grad():
                m.weight.copy_(t["weight"])
                m.bias.copy_(t["bias"])
                m.running_mean.copy_(t["running_mean"])
                m.running_var.copy_(t["running_var"])
            return m

        def run(m, x, cot):
            leaf = x.clone().requires_grad_(True)
            out = m(leaf.clone())
            kept = out.detach().clone()
            out.backward(cot)
            return kept, leaf.grad, m.weight.grad, m.bias.grad

        rows = slice(rank * per, (rank + 1) * per)
        whole, sync = module(A.InPlaceABN), module(A.InPlaceABNSync)
        w_out, w_dx, w_dw, w_db = run(whole, t["x"], t["cot"])
        s_out, s_dx, s_dw, s_db = run(sync, t["x"][rows], t["cot"][rows].contiguous())
        errs = [close(s_out, w_out[rows], "out"), close(s_dx, w_dx[rows], "dx")]
        grads = torch.stack([s_dw, s_db])
        dist.all_reduce(grads)                                    # the sum over the ranks
        errs += [close(grads[0], w_dw, "dweight"), close(grads[1], w_db, "dbias")]
        errs += [close(sync.running_mean, whole.running_mean, "running_mean"), close(sync.running_var, whole.running_var, "running_var")]
        stats = torch.stack([sync.running_mean, sync.running_var]).contiguous()
        parts = [torch.empty_like(stats) for _ in range(world)]
        dist.all_gather(parts, stats)
        for p in parts:
            assert torch.equal(p.view(torch.int32), parts[0].view(torch.int32)), "running statistics differ between ranks"
        # eval mode takes no collective: with the same running statistics it IS the plain module
        sync.eval()
        whole.eval()
        with torch.no_grad():
            whole.running_mean.copy_(sync.running_mean)
            whole.running_var.copy_(sync.running_var)
            assert torch.equal(sync(t["x"][rows].clone()), whole(t["x"].clone())[rows])
        worst = max(worst, max(errs))
        print("rank %d %s %s (%s): worst %.3g" % (rank, shape, act, regime, max(errs)), flush=True)
    dist.barrier()
    if rank == 0:
        print("ABN_SYNC_OK world=%d worst=%.3g" % (world, worst), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
