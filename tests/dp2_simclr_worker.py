"""Worker of tests/test_gpu_simclr_engine.py: one rank of a 2-rank data-parallel p = 0 engine step (SimCLRLoss, dot products) on
cuda:0 (gloo collectives on CUDA tensors, eager launches), results written to an .npz.
usage: dp2_simclr_worker.py <rank> <port> <outdir> <B> <n> <head>"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_problem(n, B_total, head):
    """Unit-sphere latents (the reference's hypersphere experiment) through an encoder with the given output head."""
    from cl_ica_amd import encoders
    torch.manual_seed(0)
    f = encoders.get_mlp(n, n, [10 * n, 50 * n, 50 * n, 10 * n], output_normalization=head).to("cuda")
    if head is None:          # keeps a fresh encoder's embeddings apart (tests/test_gpu_simclr_engine.py: collapsed rows cancel in dy)
        for m in f:
            if isinstance(m, torch.nn.Linear):
                m.weight.data.mul_(2.2)
    g = torch.Generator(device="cpu").manual_seed(1)
    gW = (torch.randn(3, n, n, generator=g) / n ** 0.5).to("cuda")
    z1 = torch.randn(B_total, n, generator=g)
    z1 = z1 / z1.norm(dim=1, keepdim=True)
    z2 = z1 + 0.05 * torch.randn(B_total, n, generator=g)
    z2 = z2 / z2.norm(dim=1, keepdim=True)
    return f, gW, z1.to("cuda"), z2.to("cuda")


def main():
    rank, port, outdir, B, n = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    head = sys.argv[6] if len(sys.argv) > 6 and sys.argv[6] != "None" else None
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    f, gW, z1, z2 = make_problem(n, 2 * B, head)
    tr = ContrastiveTrainer(f, gW, SamplerSpec(space="sphere", n=n), batch_size=B, p=0, tau=0.5, alpha=0.5, lr=0.0, device="cuda",
                            process_group=dist.group.WORLD)
    assert tr.world == 2 and tr.dp and tr.plan_summary()["loss_entry_points"] == "dot train pair"
    out = tr.step_injected(z1[rank * B:(rank + 1) * B], z2[rank * B:(rank + 1) * B])
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), means=out.cpu().numpy(), grad=tr.grad_arena.cpu().numpy(),
             loss_i=tr.loss_out[:B].cpu().numpy())
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
