"""Shader-cycle stamps of the batched streaming kernel k_vlfan_partial_dma_batch<false> (-DVLSA_TIMING): per-phase cycles of
own tile 12 of wave (rg, cw = 0) of workgroup 3, for BOTH row groups, on 64 distinct 50k bags (HBM) and on 32 bags that are
all the same tensor (cache-resident, tools/kbench_resident.py's "ONE tensor" case).

    python tools/batch_stamps.py build [OUT.so]    (no GPU: the library's objects + a -DVLSA_TIMING vlfan_batch.o)
    python tools/batch_stamps.py [LIB.so]          (GPU)

Stamps (ISTAMP in vlfan_batch.hip): 0 tile loop entry of the tile, 1 tile landed (next DMA issued), 2 score / norm MFMAs done,
3 past the first exchange sync, 4 past the second, 5 scores normalised, 6 weights formed, 7 weighted-sum MFMAs done.
Cycle counters of different waves are comparable (one CU), so rg1 - rg0 at stamp 1 is the phase offset of the two groups."""
import ctypes, glob, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBD = os.path.join(ROOT, "vlsa_amd", "_lib")
DEFAULT = os.path.join(LIBD, "variants", "libvlsa_batchtiming.so")
if len(sys.argv) > 1 and sys.argv[1] == "build":
    out = sys.argv[2] if len(sys.argv) > 2 else DEFAULT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    objs = [o for o in glob.glob(os.path.join(LIBD, "obj", "*.o")) if not o.endswith("vlfan_batch.o")]
    tobj = out + ".vlfan_batch.o"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DVLSA_TIMING", "-c",
                           os.path.join(ROOT, "vlsa_amd", "csrc", "vlfan_batch.hip"), "-o", tobj])
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, tobj, "-o", out])
    sys.exit(0)
os.environ["VLSA_HIP_LIB"] = sys.argv[1] if len(sys.argv) > 1 else DEFAULT
sys.path.insert(0, ROOT)
import torch
from vlsa_amd import _native as nat
from vlsa_amd import functional as F
dev = "cuda"
lib = nat.load()
lib.vlsa_debug_read_batch_cycles.argtypes = [ctypes.c_void_p]
buf = (ctypes.c_longlong * 64)()
NAMES = ["landed", "score MFMAs", "sync 1", "sync 2", "normalise", "weights", "wsum MFMAs"]


def case(label, B, n, alias):
    base = torch.randn((1 if alias else B) * n + 4096, 512, device=dev).to(torch.bfloat16)
    bags = [base[0:n] if alias else base[i * n:(i + 1) * n] for i in range(B)]
    Q = torch.randn(12, 512, device=dev); T = torch.randn(4, 512, device=dev)
    W = torch.randn(512, 512, device=dev) / 22; b = torch.randn(512, device=dev); ls = torch.tensor(4.03, device=dev)
    plan = F.VlfanBatchPlan(B, 12, 4, dev)
    plan.set_bags(bags); plan.run(Q, T, ls, W, b)
    for _ in range(30):
        plan.run_partial_only()
    torch.cuda.synchronize()
    rows = []
    for _ in range(9):
        plan.run_partial_only(); torch.cuda.synchronize()
        assert lib.vlsa_debug_read_batch_cycles(buf) == 0
        r0 = [buf[40 + k] for k in range(8)]
        r1 = [buf[48 + k] for k in range(8)]
        rows.append(([r0[k + 1] - r0[k] for k in range(7)], [r1[k + 1] - r1[k] for k in range(7)], r1[1] - r0[1]))
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"== {label}: B={B} N={n} groups={plan.groups}, cycles per phase (median of 9 launches)")
    for k in range(7):
        print(f"   {k}->{k + 1} {NAMES[k]:12s}  rg0 {med([r[0][k] for r in rows]):6d}   rg1 {med([r[1][k] for r in rows]):6d}")
    print(f"   total 0->7         rg0 {med([sum(r[0]) for r in rows]):6d}   rg1 {med([sum(r[1]) for r in rows]):6d}")
    print(f"   rg1 - rg0 at stamp 1 (same own tile index): {med([r[2] for r in rows])}")


with torch.no_grad():
    case("HBM, distinct bags", 64, 50000, False)
    case("resident, ONE tensor", 32, 50000, True)
