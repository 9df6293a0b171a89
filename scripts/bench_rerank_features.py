"""Row-form re-ranking from the features (ops.re_ranking_from_features, DESIGN
6.1.4) measured against the matrix path it can replace and against the same
re-ranking with the gallery prepared once (ops.RerankGallery), on
one GPU.

Duke shape (Q=2228, G=17661, D=3968, cosine, k1=20, k2=6, lambda=0.3; the
synthetic identities of scripts/bench_duke_rerank.py):
  A = ops.self_distance_blocks + ops.re_ranking(symmetric=True, whole=True)
  B = ops.re_ranking_from_features
  C = ops.RerankGallery(g) once per repetition (C_prep), then .re_rank(q) (C)
one process, the legs alternating, medians of device-event times over --reps
repetitions after a warm-up; peak allocation of each, max |A - B|, the share
of cells more than 1e-5 apart, the re-ranked mAP of A and B, and whether C
equals B bit for bit.

Large shape (B and C): Q=2,000 x G=150,000, D=256 -- its [N, N] matrix would be
92 GB and G is past the matrix path's cap of 38,400, so the gallery windows run.
Serving shape (B and C): Q=64 against the same kind of gallery.

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


def _c_legs(g, q, metric):
    """One repetition of leg C: (result, prep ms, batch ms, prep peak, batch peak)."""
    from pps_amd import ops
    rg, ms_p, peak_p = _timed(lambda: ops.RerankGallery(g, K1, metric=metric))
    c, ms_c, peak_c = _timed(lambda: rg.re_rank(q, K1, K2, LAM))
    return c, ms_p, ms_c, peak_p, peak_c


def _c_fields(tc, tp, pc, pp, tb, equal):
    return dict(C='RerankGallery(g) [C_prep], then .re_rank(q) [C]', C_ms=_median(tc),
                C_prep_ms=_median(tp), C_ms_all=[round(t, 3) for t in tc],
                C_prep_ms_all=[round(t, 3) for t in tp],
                B_over_C=round(_median(tb) / _median(tc), 3), C_peak_MB=round(pc / 1e6, 1),
                C_prep_peak_MB=round(pp / 1e6, 1), C_equals_B=equal)


def run_duke(reps):
    from pps_amd import ops
    from pps_amd import reid_dataset_evaluator as gev
    from bench_duke_rerank import NOISE, D, G, Q
    x, (qid, gid, qcam, gcam) = _features(Q, G, D, 703, NOISE, 0)
    q, g = x[:Q].contiguous(), x[Q:].contiguous()

    def path_a():
        _, q_g, q_q, g_g = ops.self_distance_blocks(x, Q, metric='cosine')
        return ops.re_ranking(q_g, q_q, g_g, K1, K2, LAM, symmetric=True, whole=True)

    def path_b():
        return ops.re_ranking_from_features(x, Q, K1, K2, LAM, metric='cosine')

    ta, tb, tc, tp, pa, pb, pc, pp = [], [], [], [], 0, 0, 0, 0
    for rep in range(reps + 1):           # rep 0 warms every leg up
        a, ms_a, peak_a = _timed(path_a)
        b, ms_b, peak_b = _timed(path_b)
        c, ms_p, ms_c, peak_p, peak_c = _c_legs(g, q, 'cosine')
        if rep:
            ta.append(ms_a)
            tb.append(ms_b)
            tc.append(ms_c)
            tp.append(ms_p)
            pa, pb, pc, pp = max(pa, peak_a), max(pb, peak_b), max(pc, peak_c), max(pp, peak_p)
        if rep < reps:
            del a, b, c
    diff = (a - b).abs()
    mAP_a = gev.scores_from_ranks(*gev.rank_eval(a, qid, gid, qcam, gcam))[0]
    mAP_b = gev.scores_from_ranks(*gev.rank_eval(b, qid, gid, qcam, gcam))[0]
    N = Q + G
    res = dict(shape='Duke Q=%d G=%d D=%d cosine (%d, %d, %g)' % (Q, G, D, K1, K2, LAM),
               math=ops.dist_math(), reps=reps, feature_noise=NOISE,
               A='self_distance_blocks + re_ranking(whole=True)', B='re_ranking_from_features',
               A_ms=_median(ta), B_ms=_median(tb), A_ms_all=[round(t, 3) for t in ta],
               B_ms_all=[round(t, 3) for t in tb], B_over_A=round(_median(tb) / _median(ta), 3),
               A_peak_MB=round(pa / 1e6, 1), B_peak_MB=round(pb / 1e6, 1),
               matrix_MB=round(4.0 * N * N / 1e6, 1), max_abs_diff=float(diff.max()),
               share_over_1e5=float((diff > 1e-5).float().mean()),
               mAP_A=round(float(mAP_a), 6), mAP_B=round(float(mAP_b), 6))
    res.update(_c_fields(tc, tp, pc, pp, tb, bool(torch.equal(b, c))))
    res['C_over_A'] = round(_median(tc) / _median(ta), 3)
    return res


def run_large(reps, Q=2000, G=150000, D=256):
    """B and C alternating at a gallery past the matrix path's cap."""
    from pps_amd import ops
    x, _ = _features(Q, G, D, 5000, 2.5, 1)
    q, g = x[:Q].contiguous(), x[Q:].contiguous()
    tb, tc, tp, pb, pc, pp = [], [], [], 0, 0, 0
    finite = equal = True
    for rep in range(reps + 1):
        b, ms_b, peak_b = _timed(lambda: ops.re_ranking_from_features(x, Q, K1, K2, LAM))
        c, ms_p, ms_c, peak_p, peak_c = _c_legs(g, q, 'euclidean')
        if rep:
            tb.append(ms_b)
            tc.append(ms_c)
            tp.append(ms_p)
            pb, pc, pp = max(pb, peak_b), max(pc, peak_c), max(pp, peak_p)
        finite = finite and bool(torch.isfinite(b).all())
        equal = equal and bool(torch.equal(b, c))
        del b, c
    N = Q + G
    res = dict(shape='Q=%d G=%d D=%d euclidean (%d, %d, %g)' % (Q, G, D, K1, K2, LAM),
               reps=reps, B_ms=_median(tb), B_ms_all=[round(t, 3) for t in tb],
               B_peak_MB=round(pb / 1e6, 1), matrix_MB=round(4.0 * N * N / 1e6, 1),
               gallery_windows=-(-G // 38400), finite=finite)
    res.update(_c_fields(tc, tp, pc, pp, tb, equal))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--large-reps', type=int, default=None, help='default: --reps')
    ap.add_argument('--skip-large', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON here')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rerank_features: no GPU (there is no CPU path to time)')
    res = dict(duke=run_duke(a.reps))
    if not a.skip_large:
        large_reps = a.reps if a.large_reps is None else a.large_reps
        res['large'] = run_large(large_reps)
        res['serving'] = run_large(large_reps, Q=64)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
