"""What ``CE.graph`` costs next to the forward of the same call (a diagnostic path: the number is for users, not a target).

    python tools/time_patch_graph.py [H W]          # default 256 256: top-k 8 and the dense adaptive regime
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    from dagl_amd.ce import CE
    from dagl_amd.synth import make_ce_params, make_features
    H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 256)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(make_features(7, 1, 64, H, W)).to(dev)
    for mode, k, variant in (("topk", 8, "default"), ("adaptive", 0, "default"), ("adaptive", 0, "sparse")):
        prm = {n: torch.from_numpy(a) for n, a in make_ce_params(7, variant=variant, sparse_gain=1.65).items()}
        ce = CE(in_channels=64)
        ce.load_state_dict(prm, strict=True)
        ce.select_mode, ce.select_k = mode, max(k, 1)
        ce = ce.to(dev).eval()
        with torch.no_grad():
            fwd = _timed(lambda: ce(x), 10)
            deg = _timed(lambda: ce.degrees(x), 3)
            holder = {}
            def export():
                holder["g"] = None                      # (release the previous arrays first)
                holder["g"] = ce.graph(x)
            tot = _timed(export, 3)
        g = holder["g"]
        print(f"[1,64,{H},{W}] {mode} k={k} ({variant}): {g.n_edges} edges (mean degree {g.n_edges / g.L:.1f}); "
              f"graph {tot:.2f} ms, degrees alone {deg:.2f} ms, forward {fwd:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
