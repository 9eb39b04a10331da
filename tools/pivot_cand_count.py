"""Run ON THE GPU BOX: candidates per query of the top-k filter pass (k = 8, 256 x 256) under the two sampled thresholds -- every 8th
key tile against the pivot keys the library picked (read back through dagl_ce_pivot_debug) -- on bench.py's synthetic map and on one
Set12 feature map.  Scores are formed here (bf16 operands, fp32 sums); the grouping is the sampling launch's: per (key chunk, lane half)
the four largest of sixteen group maxima, theta = the k-th largest of those less the band."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, torch.nn.functional as F
from dagl_amd import ops
from dagl_amd.ce import CE
from dagl_amd.synth import make_ce_params, make_features
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"); dev = torch.device("cuda:0")
DELTA, K = 0.0079, 8
def rows(ce, x):
    with torch.no_grad():
        b1 = ce.g(x)
        X = F.relu(ce.fc2(F.unfold(F.pad(b1, (3, 3, 3, 3)), 7).transpose(1, 2)[0]))
        Q = F.relu(ce.fc1(F.unfold(F.pad(b1, (1, 2, 1, 2)), 7, stride=4).transpose(1, 2)[0]))
    return Q, X
def theta_of(Sb, step, row, split, sampled, nsplit):
    h = (row >> 2) & 1; r = (row & 3) + 4 * ((row & 31) >> 3)
    gid = ((split * 2 + h) * 16 + r)[sampled]
    gm = torch.full((Sb.shape[0], nsplit * 2 * 16), -1.0, device=dev)
    gm.scatter_reduce_(1, gid.expand(Sb.shape[0], -1), Sb, reduce="amax")
    kept = gm.view(Sb.shape[0], nsplit * 2, 16).topk(4, dim=2).values.reshape(Sb.shape[0], -1)
    kth = kept.topk(K, dim=1).values[:, -1:]
    return torch.where(kth > 0, kth * ((1 - DELTA) / (1 + DELTA)), torch.zeros_like(kth))
def report(label, ce, x):
    Q, X = rows(ce, x)
    N = X.shape[0]
    ce.select_mode, ce.select_k, ce.topk_threshold = "topk", K, "sparse"
    with torch.no_grad():
        ce(x)
    idx, _ = ops.ce_pivot_debug(x.shape, "topk", K, ce._ws, dev)
    idx = idx[0].long()                                              # [n_blk, 2]
    n_blk = idx.shape[0]; steps = (n_blk + 31) // 32
    Qb, Xb = Q.to(torch.bfloat16).float(), X.to(torch.bfloat16).float()
    n = torch.arange(N, device=dev); step = n // 64
    old_sampled = (step % 32) % 8 == 0
    v = torch.arange(n_blk, device=dev)
    prow = (2 * (v // steps))[:, None] + torch.arange(2, device=dev)[None]          # row of the pivot inside its step
    pstep = (v % steps)[:, None].expand(-1, 2)
    nsplit = 32; sps = (steps + nsplit - 1) // nsplit
    out = {"every 8th tile": [], "pivots": []}
    for q0 in range(0, Q.shape[0], 512):
        S = Qb[q0:q0 + 512] @ Xb.t()
        th_old = theta_of(S[:, old_sampled], step, n % 64, step // 32, old_sampled, nsplit)
        ok = (idx >= 0).reshape(-1)
        Sp = S[:, idx.reshape(-1).clamp(min=0)][:, ok]
        th_new = theta_of(Sp, pstep.reshape(-1)[ok], prow.reshape(-1)[ok], (pstep // sps).reshape(-1)[ok], torch.ones(int(ok.sum()), dtype=torch.bool, device=dev), nsplit)
        out["every 8th tile"].append((S >= th_old).sum(1)); out["pivots"].append((S >= th_new).sum(1))
    for name, c in out.items():
        c = torch.cat(c).float()
        print(f"{label:24s} {name:15s}: candidates per query mean {c.mean():7.1f} p99 {c.quantile(0.99):6.0f} max {int(c.max()):5d}", flush=True)
prm = {n: torch.from_numpy(a) for n, a in make_ce_params(2024, variant="default").items()}
ce = CE(in_channels=64); ce.load_state_dict(prm, strict=True); ce = ce.to(dev).eval()
report("bench map (seed 100)", ce, torch.from_numpy(make_features(100, 1, 64, 256, 256)).to(dev))
if "--set12" in sys.argv:
    from dagl_amd.net import RR, set12_protocol_noise
    z = np.load(os.path.join(G, "quality_ckpt_fp16.npz"))
    net = RR().eval(); net.load_state_dict({k: torch.from_numpy(z[k].astype(np.float32)) for k in z.files}, strict=True); net = net.to(dev)
    imgs = np.load(os.path.join(G, "set12.npz"))
    clean = torch.from_numpy(imgs["img_01"].astype(np.float32) / 255.0)[None, None]
    noisy = set12_protocol_noise(clean, 50.0, 1.0).to(dev)
    with torch.no_grad():
        x = net.head(noisy)
        for blk in net.body[:8]: x = blk(x)
    report("Set12 img_01, body[8]", net.body[8].c1_1, x.contiguous())
