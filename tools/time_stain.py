#!/usr/bin/env python3
"""Times the stain kernels on one GPU beside the same arithmetic written in torch on the device:

  (i)   `mil_stain_affine_u8` alone, by default on 500 tiles of 300 x 300 with one map per tile (and with one shared map), every
        argument already on the device; `apply_stain`, which adds the host side of a call (the fp64 -> fp32 parameters and
        their upload); and the torch chain  u8 -> float -> log -> matmul -> exp -> round -> clamp -> uint8;
  (ii)  the three launches of a Macenko fit, by default on 256 tiles of 256 x 256: `ops.od_moments` (bag), `ops.od_project`
        ratio and concentrations, the four `ops.map_quantile` calls a fit makes, the whole `StainNormalizer.fit` with its host
        steps and read-backs; and torch's masked moments (fp64 sums of fp32 log) and projections (matmul + where).

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of (i) are one read
and one write of the stack; its rate is printed next to the 8 TB/s HBM peak.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L, ops  # noqa: E402
from mil_amd import stain as st  # noqa: E402

HBM_PEAK_TBPS = 8.0


def timed(f, warmup, reps, before=None):
    out = []
    for it in range(warmup + reps):
        if before is not None:
            before()                      # untimed: every repetition maps the same bytes
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def he_like(t, r, seed):
    """uint8 [t,3,r,r] on the GPU: one synthetic H&E tile — a quarter background, the rest random amounts of the reference
    fit's two stains with OD noise — repeated (the kernels' time does not depend on the bytes beyond the tissue share)."""
    rng = np.random.default_rng(seed)
    conc = rng.uniform(0.0, 1.6, (r * r, 2)) * (rng.integers(0, 4, (r * r, 1)) > 0)
    od = conc @ mil_amd.StainFit.reference().stains.T + rng.normal(0.0, 0.01, (r * r, 3))
    one = np.clip(np.rint(256.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8).T.reshape(1, 3, r, r)
    return torch.from_numpy(np.ascontiguousarray(one)).cuda().expand(t, 3, r, r).contiguous()


def torch_affine(u8, A, b):
    od = -torch.log((u8.float() + 1.0) / 256.0)                                  # [T,3,H,W]
    o = torch.einsum("tij,tjhw->tihw", A, od) + b[:, :, None, None]
    return torch.round(256.0 * torch.exp(-o) - 1.0).clamp_(0.0, 255.0).to(torch.uint8)


def torch_moments(u8, beta):
    od = -torch.log((u8.float() + 1.0) / 256.0)
    m = (od >= beta).all(dim=1, keepdim=True)
    x = (od * m).permute(1, 0, 2, 3).reshape(3, -1).double()
    return m.sum(), x.sum(dim=1), x @ x.t()


def torch_project(u8, P, beta, ratio):
    od = -torch.log((u8.float() + 1.0) / 256.0)
    m = (od >= beta).all(dim=1)
    p = torch.einsum("kj,tjhw->kthw", P, od)
    inf = torch.full((), float("inf"), device=u8.device)
    if ratio:
        return torch.where(m & (p[0] > 0), p[1] / p[0], inf)
    return torch.where(m[None], p, inf)


def torch_snmf_iteration(u8, W, lam, beta):
    """One iteration of the sparse factorisation in torch ops: the closed-form code in fp32, the sums in fp64, the update."""
    od = -torch.log((u8.float() + 1.0) / 256.0)
    m = (od >= beta).all(dim=1)
    Wf = W.float()
    c = W[:, 0] @ W[:, 1]                                                 # stays on the device: no synchronisation
    c, d = c.float(), (1.0 / (1.0 - c * c)).float()
    q = torch.einsum("jk,tjhw->kthw", Wf, od) - lam
    h0, h1 = (q[0] - c * q[1]) * d, (q[1] - c * q[0]) * d
    both, zero = (h0 >= 0) & (h1 >= 0), torch.zeros((), device=u8.device)
    a0 = torch.where(both, h0, torch.where(h1 < 0, q[0].clamp_min(0), zero))
    a1 = torch.where(both, h1, torch.where(h1 < 0, zero, q[1].clamp_min(0)))
    H = (torch.stack([a0, a1]) * m[None]).reshape(2, -1).double()
    V = (od * m[:, None]).permute(1, 0, 2, 3).reshape(3, -1).double()
    A, B = H @ H.t(), V @ H.t()
    W = W.clone()
    for j in (0, 1):
        u = (W[:, j] + (B[:, j] - W @ A[:, j]) / A[j, j]).clamp_min(0)
        W[:, j] = u / u.norm()
    return W, H.sum(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=500)
    ap.add_argument("--resolution", type=int, default=300)
    ap.add_argument("--fit-tiles", type=int, default=256)
    ap.add_argument("--fit-resolution", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--snmf-iters", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_stain.py needs a GPU")
    lib = L.lib()
    times = {}

    # (i) the affine map
    t, r = a.tiles, a.resolution
    src = he_like(t, r, 1)
    work = src.clone()
    jit = mil_amd.StainJitter(0.05, 0.01)
    aff = jit.affine(jit.draw_params(t, torch.Generator().manual_seed(1)))
    per_tile, shared = aff.params().cuda(), aff.params()[:1].cuda()
    tab = ops.od_tables("cuda")

    def launch(p, sh):
        return lambda: L.check(lib.mil_stain_affine_u8(work.data_ptr(), p.data_ptr(), tab.data_ptr(), t, r, r, sh, L.stream_ptr()),
                               "mil_stain_affine_u8")

    def restore():
        work.copy_(src)

    times["affine_launch_per_tile"] = timed(launch(per_tile, 0), a.warmup, a.reps, restore)
    times["affine_launch_shared"] = timed(launch(shared, 1), a.warmup, a.reps, restore)
    handle = mil_amd.U8Tiles(work)
    times["affine_apply_stain"] = timed(lambda: st.apply_stain(handle, aff), a.warmup, a.reps, restore)
    A32, b32 = torch.from_numpy(aff.A).float().cuda(), torch.from_numpy(aff.b).float().cuda()
    times["affine_torch_chain"] = timed(lambda: torch_affine(src, A32, b32), a.warmup, a.reps)
    got = st.apply_stain(mil_amd.U8Tiles(src.clone()), aff).u8
    diff = (got.int() - torch_affine(src, A32, b32).int()).abs()
    del work, handle, got

    # (ii) the launches of a fit
    ft, fr = a.fit_tiles, a.fit_resolution
    tiles = mil_amd.U8Tiles(he_like(ft, fr, 2))
    norm = mil_amd.StainNormalizer()
    fit = norm.fit(tiles)
    P1 = torch.from_numpy(st.fit_plane(ops.od_moments(tiles.u8, 0.15, "bag")[0].cpu().numpy())).float().cuda()
    P2 = torch.from_numpy(np.linalg.pinv(fit.stains)).float().cuda()
    times["fit_od_moments_bag"] = timed(lambda: ops.od_moments(tiles.u8, 0.15, "bag"), a.warmup, a.reps)
    times["fit_od_project_ratio"] = timed(lambda: ops.od_project(tiles.u8, P1.cpu(), "ratio", 0.15), a.warmup, a.reps)
    times["fit_od_project_concentrations"] = timed(lambda: ops.od_project(tiles.u8, P2.cpu(), "concentrations", 0.15), a.warmup, a.reps)
    ratio = ops.od_project(tiles.u8, P1.cpu(), "ratio", 0.15)[0]
    times["fit_four_map_quantiles"] = timed(lambda: [ops.map_quantile(ratio, q, "bag") for q in (0.5, 49.0, 49.5, 49.9)], a.warmup, a.reps)
    times["fit_whole"] = timed(lambda: norm.fit(tiles), a.warmup, a.reps)
    times["fit_torch_moments"] = timed(lambda: torch_moments(tiles.u8, 0.15), a.warmup, a.reps)
    times["fit_torch_project_ratio"] = timed(lambda: torch_project(tiles.u8, P1, 0.15, True), a.warmup, a.reps)
    times["fit_torch_project_concentrations"] = timed(lambda: torch_project(tiles.u8, P2, 0.15, False), a.warmup, a.reps)

    # (iii) Vahadane's fit on the same stack
    W0 = st.HED[:, :2].copy()
    vnorm = mil_amd.StainNormalizer(method="vahadane", iters=a.snmf_iters)
    times["snmf_sums_pass"] = timed(lambda: ops.od_snmf_sums(tiles.u8, W0, 0.1, 0.15), a.warmup, a.reps)
    times["snmf_fit_device_loop"] = timed(lambda: ops.od_snmf_fit(tiles.u8, W0, 0.1, a.snmf_iters, 0.15), a.warmup, a.reps)
    times["snmf_fit_whole"] = timed(lambda: vnorm.fit(tiles), a.warmup, a.reps)
    Wt = torch.from_numpy(W0).cuda()
    times["snmf_torch_one_iteration"] = timed(lambda: torch_snmf_iteration(tiles.u8, Wt, 0.1, 0.15), a.warmup, a.reps)
    vfit = vnorm.fit(tiles)

    moved = 2 * t * 3 * r * r
    res = {"tiles": t, "resolution": r, "fit_tiles": ft, "fit_resolution": fr, "affine_algorithmic_bytes": moved, "reps": a.reps,
           "library": os.path.basename(mil_amd.LIB_PATH), "fit_n_tissue": fit.n_tissue,
           "affine_vs_torch_chain": {"largest_byte_difference": int(diff.max()), "share_differing": float((diff != 0).float().mean())},
           "snmf_iters": a.snmf_iters, "snmf_last_move": vfit.last_move}
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    tbps = moved / statistics.median(times["affine_launch_per_tile"]) / 1e9
    res["affine_launch_per_tile"]["TBps_at_median"] = round(tbps, 3)
    res["affine_launch_per_tile"]["fraction_of_hbm_peak"] = round(tbps / HBM_PEAK_TBPS, 4)
    res["torch_chain_over_affine_launch"] = round(res["affine_torch_chain"]["median_ms"] / res["affine_launch_per_tile"]["median_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
