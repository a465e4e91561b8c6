"""Times rigid co-registration by mutual information (csrc/coreg.hip, bts_amd.coreg) on a 240x240x155 scan at 1 mm: one evaluation of
K = 13 candidates at each of the two default lattices (strides 4 and 2), and a whole default registration; and the same arithmetic in
numpy (tests/coreg_ref.py) on the host, in the same run.  Prints one JSON line.

    python scripts/bench_coreg.py [--runs 50] [--warmup 5] [--no-host-registration]

The volumes are the analytic phantom of tests/coreg_ref.py, the moving one on a 232x248x150 grid at (1.05, 0.95, 1.1) mm and off by
(5, -4, 3) mm and (3, -2, 4) degrees.  `kernel_ms` is HIP events on the launch stream around one ops.joint_hist_pv call (the zeroing launch
and the histogram launch), the median of --runs after --warmup, each run with the next of 13-candidate sets of a sweep around a different
point, so that no run repeats the one before; `evaluate_ms` is the host's wall clock around the same call, the read-back of the K x 8 KB
and the 13 scores, i.e. what one sweep of the search costs.  `points` counts lattice points x candidates; every one of them inside the
moving volume gathers 8 bytes.  The registration is timed by the host's clock from the volumes on the device to the result (percentiles,
binning, every sweep), after one warm-up registration.  The numpy figures are one evaluation each and one whole registration through the
same `coreg.coregister` with the numpy evaluator; the two registrations must agree in every parameter."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FIXED, FIXED_MM = (240, 240, 155), (1.0, 1.0, 1.0)
MOVING, MOVING_MM = (232, 248, 150), (1.05, 0.95, 1.1)
POSE = (5.0, -4.0, 3.0, 3.0, -2.0, 4.0)


def sweep(p, step_mm, step_deg):
    out = [tuple(p)]
    for i in range(6):
        for sgn in (1.0, -1.0):
            q = list(p)
            q[i] += sgn * (step_mm if i < 3 else step_deg)
            out.append(tuple(q))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-host-registration', action='store_true', help='skip the whole registration in numpy (about a minute)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import coreg, ops
    import coreg_ref as R
    if not torch.cuda.is_available():
        raise SystemExit('bench_coreg.py measures on the GPU; none is available')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    a_f = R.grid_affine(FIXED, FIXED_MM)
    centre = (a_f @ np.array([(n - 1) // 2 for n in FIXED] + [1.0]))[:3]
    truth = coreg.rigid_matrix(POSE, centre)
    f, a_f, m, a_m = R.phantom_pair(FIXED, FIXED_MM, MOVING, MOVING_MM, truth)
    fg, mg = torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev)
    qf, qm = coreg._binned(fg, 32, 'fixed'), coreg._binned(mg, 32, 'moving')
    qfh, qmh = qf.cpu().numpy(), qm.cpu().numpy()
    inv_m = np.linalg.inv(a_m)
    out = {'runs': args.runs, 'warmup': args.warmup, 'fixed': FIXED, 'moving': MOVING, 'bins': 32}
    for mm, step_mm, step_deg, _ in coreg.DEFAULT_LEVELS:
        origin, stride, counts = coreg.lattice(FIXED, a_f, mm)
        sets = [np.stack([(inv_m @ coreg.rigid_matrix(p, centre) @ a_f)[:3] for p in sweep((0.5 * k, -0.25 * k, 0.0, 0.0, 0.1 * k, 0.0), step_mm, step_deg)])
                for k in range(8)]
        for k in range(args.warmup):
            ops.joint_hist_pv(qf, qm, origin, stride, counts, sets[k % 8], 32)
        torch.cuda.synchronize()
        kernel, whole = [], []
        for k in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h = ops.joint_hist_pv(qf, qm, origin, stride, counts, sets[k % 8], 32)
            b.record()
            b.synchronize()
            kernel.append(a.elapsed_time(b))
        for k in range(args.runs):
            t0 = time.perf_counter()
            h = ops.joint_hist_pv(qf, qm, origin, stride, counts, sets[k % 8], 32).cpu().numpy()
            scores = [coreg.score(x, int(np.prod(counts))) for x in h]
            whole.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ref = R.joint_hist_pv(qfh, qmh, origin, stride, counts, sets[(args.runs - 1) % 8], 32)
        host_ms = 1e3 * (time.perf_counter() - t0)
        if not np.array_equal(ref, h):
            raise SystemExit('the device histogram differs from the numpy restatement')
        pts = int(np.prod(counts)) * 13
        ms = statistics.median(kernel)
        out['evaluate_13_stride_%d' % stride[0]] = {
            'lattice': counts, 'points': pts, 'overlap': round(float(h.sum()) / 32 ** 3 / pts, 3), 'kernel_ms': round(ms, 4),
            'best_ms': round(min(kernel), 4), 'worst_ms': round(max(kernel), 4), 'Gpoints_per_s': round(pts / ms / 1e6, 2),
            'evaluate_ms': round(statistics.median(whole), 4), 'host_numpy_ms': round(host_ms, 1), 'host_over_device': round(host_ms / ms, 1),
            'scores': len(scores)}
    coreg.coregister(fg, a_f, mg, a_m)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = coreg.coregister(fg, a_f, mg, a_m)
        times.append(1e3 * (time.perf_counter() - t0))
    out['registration'] = {'ms': round(statistics.median(times), 1), 'evaluations': r.evaluations, 'sweeps': len(r.trace),
                           'params': [round(v, 4) for v in r.params], 'truth': POSE, 'nmi_before': round(r.nmi_before, 6),
                           'nmi_after': round(r.nmi_after, 6), 'mean_tre_voxel': round(R.mean_tre(r.matrix, truth, FIXED, a_f), 4),
                           'mean_tre_voxel_headers_alone': round(R.mean_tre(np.eye(4), truth, FIXED, a_f), 4)}
    if not args.no_host_registration:
        t0 = time.perf_counter()
        rh = coreg.coregister(fg, a_f, mg, a_m, evaluate=R.joint_hist_pv)
        out['registration']['host_numpy_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
        out['registration']['host_over_device'] = round(out['registration']['host_numpy_ms'] / out['registration']['ms'], 1)
        if rh.params != r.params or rh.trace != r.trace:
            raise SystemExit('the device registration differs from the numpy one')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
