"""Time DSMIL (vlsa_amd.deepmil.DSMIL.forward_bags, csrc/dsmil.hip) against the reference formula in torch on the same GPU and against
the HBM bound of the passes it makes (2 reads of the bags forward, 1 more backward).

    python tools/kbench_dsmil.py [--iters 10] [--classes 4]

Workloads: 64 x 50 000-row and 256 x 2 798-row bf16 bags, forward (no_grad, eval) and forward + backward (train, drop_rate 0.25).
The torch leg is the reference's forward (model/deepmil.py:673-713) written out below, bag by bag, fp32 on the bf16 rows' values."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12      # B/s, MI355X data sheet


def torch_dsmil(x, P, drop_p, training):
    Wc, bc, Wq, bq, Wv, bv, Wf, bf = P
    x = x.float()
    c = x @ Wc.t() + bc
    V = torch.nn.functional.dropout(x, drop_p, training) @ Wv.t() + bv
    Q = x @ Wq.t() + bq
    m = torch.sort(c, 0, descending=True)[1][0]
    qmax = x[m] @ Wq.t() + bq
    A = torch.softmax(Q @ qmax.t() / Q.shape[1] ** 0.5, 0)
    Bm = A.t() @ V
    return 0.5 * (torch.nn.functional.conv1d(Bm[None], Wf, bf).view(1, -1) + c.max(dim=0).values)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--classes", type=int, default=4)
    a = ap.parse_args()
    from vlsa_amd import functional as VF
    from vlsa_amd.deepmil import DSMIL
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=a.classes, use_feat_proj=False, drop_rate=0.25).to(dev)
    P = [m.i_classifier.fc[0].weight, m.i_classifier.fc[0].bias, m.b_classifier.q.weight, m.b_classifier.q.bias,
         m.b_classifier.v[1].weight, m.b_classifier.v[1].bias, m.b_classifier.fcc.weight, m.b_classifier.fcc.bias]
    print(f"# {torch.cuda.get_device_name(0)}, num_cls {a.classes}, {a.iters} iterations per figure, HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s")
    print(f"{'workload':>16s} {'mode':>8s} {'hip ms':>9s} {'torch ms':>9s} {'speed-up':>8s} {'HBM-bound ms':>12s} {'of bound':>8s}")
    for B, N in ((64, 50000), (256, 2798)):
        bags = VF.BagSet([torch.nn.functional.normalize(torch.randn(N, 512, device=dev), dim=1).bfloat16() for _ in range(B)])
        G = torch.randn(B, a.classes, device=dev)
        bytes_once = B * N * 512 * 2

        def hip_fwd():
            with torch.no_grad():
                return m.forward_bags(bags)

        def hip_train():
            m.zero_grad(set_to_none=True)
            (m.forward_bags(bags) * G).sum().backward()

        def torch_fwd():
            with torch.no_grad():
                return torch.cat([torch_dsmil(x, P, 0.25, False) for x in bags])

        def torch_train():
            m.zero_grad(set_to_none=True)
            (torch.cat([torch_dsmil(x, P, 0.25, True) for x in bags]) * G).sum().backward()
        for mode, hip, ref, passes in (("fwd", hip_fwd, torch_fwd, 2), ("fwd+bwd", hip_train, torch_train, 3)):
            m.train(mode != "fwd")
            th, tt = timed(hip, a.iters), timed(ref, max(2, a.iters // 3))
            bound = passes * bytes_once / HBM_PEAK * 1e3
            print(f"{B:>5d} x {N:<8d} {mode:>8s} {th:9.3f} {tt:9.3f} {tt / th:8.2f} {bound:12.3f} {bound / th:8.2f}")


if __name__ == "__main__":
    main()
