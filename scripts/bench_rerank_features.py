"""Row-form re-ranking from the features (ops.re_ranking_from_features, DESIGN
6.1.4) measured against the matrix path it can replace, on one GPU.

Duke shape (Q=2228, G=17661, D=3968, cosine, k1=20, k2=6, lambda=0.3; the
synthetic identities of scripts/bench_duke_rerank.py):
  A = ops.self_distance_blocks + ops.re_ranking(symmetric=True, whole=True)
  B = ops.re_ranking_from_features
one process, A and B alternating, medians of device-event times over --reps
repetitions after a warm-up; peak allocation of each, max |A - B|, the share
of cells more than 1e-5 apart and the re-ranked mAP of both.

Large shape (B only): Q=2,000 x G=150,000, D=256 -- its [N, N] matrix would be
92 GB and G is past the matrix path's cap of 38,400, so the gallery windows run.

  python scripts/bench_rerank_features.py [--reps 7] [--out profiles/rerank/NAME.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

K1, K2, LAM = 20, 6, 0.3


def _features(Q, G, D, n_ids, noise, seed):
    rng = np.random.RandomState(seed)
    qid, gid = rng.randint(1, n_ids, Q), rng.randint(1, n_ids, G)
    qcam, gcam = rng.randint(1, 9, Q), rng.randint(1, 9, G)
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    cent = torch.randn((n_ids, D), generator=gen, device='cuda')
    ids = torch.from_numpy(np.concatenate([qid, gid])).cuda()
    x = cent[ids] + noise * torch.randn((Q + G, D), generator=gen, device='cuda')
    return (x / x.norm(dim=1, keepdim=True)).contiguous(), (qid, gid, qcam, gcam)


def _timed(fn):
    """(result, ms from device events, peak bytes allocated above the entry level)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base


def _median(v):
    return round(sorted(v)[len(v) // 2], 3)


def run_duke(reps):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    from bench_duke_rerank import NOISE, D, G, Q
    x, (qid, gid, qcam, gcam) = _features(Q, G, D, 703, NOISE, 0)

    def path_a():
        _, q_g, q_q, g_g = ops.self_distance_blocks(x, Q, metric='cosine')
        return ops.re_ranking(q_g, q_q, g_g, K1, K2, LAM, symmetric=True, whole=True)

    def path_b():
        return ops.re_ranking_from_features(x, Q, K1, K2, LAM, metric='cosine')

    ta, tb, pa, pb = [], [], 0, 0
    for rep in range(reps + 1):           # rep 0 warms both up
        a, ms_a, peak_a = _timed(path_a)
        b, ms_b, peak_b = _timed(path_b)
        if rep:
            ta.append(ms_a)
            tb.append(ms_b)
            pa, pb = max(pa, peak_a), max(pb, peak_b)
        if rep < reps:
            del a, b
    diff = (a - b).abs()
    mAP_a = gev.scores_from_ranks(*gev.rank_eval(a, qid, gid, qcam, gcam))[0]
    mAP_b = gev.scores_from_ranks(*gev.rank_eval(b, qid, gid, qcam, gcam))[0]
    N = Q + G
    return dict(shape='Duke Q=%d G=%d D=%d cosine (%d, %d, %g)' % (Q, G, D, K1, K2, LAM),
                math=ops.dist_math(), reps=reps, feature_noise=NOISE,
                A='self_distance_blocks + re_ranking(whole=True)', B='re_ranking_from_features',
                A_ms=_median(ta), B_ms=_median(tb), A_ms_all=[round(t, 3) for t in ta],
                B_ms_all=[round(t, 3) for t in tb], B_over_A=round(_median(tb) / _median(ta), 3),
                A_peak_MB=round(pa / 1e6, 1), B_peak_MB=round(pb / 1e6, 1),
                matrix_MB=round(4.0 * N * N / 1e6, 1), max_abs_diff=float(diff.max()),
                share_over_1e5=float((diff > 1e-5).float().mean()),
                mAP_A=round(float(mAP_a), 6), mAP_B=round(float(mAP_b), 6))


def run_large(reps):
    from pps_amd import ops
    Q, G, D = 2000, 150000, 256
    x, _ = _features(Q, G, D, 5000, 2.5, 1)
    tb, pb = [], 0
    for rep in range(reps + 1):
        b, ms_b, peak_b = _timed(lambda: ops.re_ranking_from_features(x, Q, K1, K2, LAM))
        if rep:
            tb.append(ms_b)
            pb = max(pb, peak_b)
        finite = bool(torch.isfinite(b).all())
        del b
    N = Q + G
    return dict(shape='Q=%d G=%d D=%d euclidean (%d, %d, %g)' % (Q, G, D, K1, K2, LAM),
                reps=reps, B_ms=_median(tb), B_ms_all=[round(t, 3) for t in tb],
                B_peak_MB=round(pb / 1e6, 1), matrix_MB=round(4.0 * N * N / 1e6, 1),
                gallery_windows=-(-G // 38400), finite=finite)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--large-reps', type=int, default=3)
    ap.add_argument('--skip-large', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON here')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rerank_features: no GPU (there is no CPU path to time)')
    res = dict(duke=run_duke(a.reps))
    if not a.skip_large:
        res['large'] = run_large(a.large_reps)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
