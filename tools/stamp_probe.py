import os, sys, ctypes as C, numpy as np, torch
sys.path.insert(0, "/root/repo")
from dr4sr_amd import _lib
from dr4sr_amd.engine import SasrecEngine
from dr4sr_amd.data.synthetic import make_rows, TOYS_N_ITEMS
import bench
lib = _lib.load()
dev = torch.device("cuda", 0)
B, L, D, H, F, NL, N = 256, 50, 64, 2, 128, 2, TOYS_N_ITEMS
rows = make_rows(n_items=N, seed=2024, dense=bool(int(os.environ.get("DENSE", "0"))))
data = {k: torch.from_numpy(rows[k]).to(dev) for k in ("in_item_id", "item_id", "seqlen")}
eng = SasrecEngine(N, L, D, H, F, NL, 1e-12, 0.5, B, dev, seed=2023)
bench.init_params_like_reference(eng, 2023)
rb = torch.arange(B, device=dev)
neg = torch.zeros(B, L, dtype=torch.int64, device=dev)
plan = eng.make_plan(data["in_item_id"], data["item_id"], data["seqlen"], rows=rb, neg_item=neg, sample_neg=True)
for _ in range(3):
    eng.train_step(plan)
torch.cuda.synchronize()
Tmax = B * L
r = lambda nfl: (nfl * 4 + 255) // 256 * 256
off = r(B + 1) + r((Tmax + 15) // 16 + 1) + r(4 + 7 * B) + r(4 * B + 4 * 1024) + r(Tmax * H) + 2 * (NL + 1) * r(Tmax * D)      # csrc/step.hip carve_workspace: ... -> dctx
os.environ["DR4SR_STAMPS"] = "1"
lib.dr4sr_reload_env()                                 # the library caches its switches per process
# phase boundaries (STAMP / TSTAMP indices of csrc/linear.hip and csrc/attn_tile.h, workgroup 0 thread 0), experiments build only:
#   forward body  0 entry | 1 attention + out_proj fragments | 2 out_proj | 3 LN1 row pass | 4 linear1 | 5 GELU pass | 6 linear2 | 15 LN2 row pass (+ next in_proj)
#   backward body 16 entry requests + attention keep bits | 17 LN2' / dh / da / dy / LN1' / dctx (the three row passes and four GEMMs) |
#                 18 far rows | 20..22 attention backward | 26 end
FWD = [0, 1, 2, 3, 4, 5, 6, 15]
BWD = [16, 17, 18, 20, 21, 22, 26]
for kind, layer, idx in (("post_fwd", 0, FWD), ("post_mid", NL - 1, FWD + BWD), ("post_bwd", 0, BWD)):
    kid = _lib.KERNEL_IDS[kind]
    eng.workspace[off:off + 32 * 8].zero_()
    for _ in range(3):
        _lib.check(lib.dr4sr_sasrec_launch_kernel(C.byref(plan), kid, layer, _lib.cur_stream()), kind)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        _lib.check(lib.dr4sr_sasrec_launch_kernel(C.byref(plan), kid, layer, _lib.cur_stream()), kind)
    b.record(); b.synchronize()
    st = eng.workspace[off:off + 32 * 8].view(torch.int64).cpu().numpy()
    assert st[idx[-1]] > st[idx[0]], "stamp buffer offset is stale (or not the experiments build: DR4SR_LIB_PATH)"
    d = np.diff(st[idx])
    print(kind, layer, "us/launch %.2f" % (a.elapsed_time(b) * 1e3 / 20), "stamps", idx, "phase ticks", d.tolist(), "total", int(st[idx[-1]] - st[idx[0]]))
