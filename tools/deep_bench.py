#!/usr/bin/env python3
"""Measurement of the DEEP step at the C3 shape (256 columns, n = 2^22, D = 4): the evaluations at
z over coset 0 (bj_evaluate_at_d, prover.rs:1501-1780) and one opening point of the quotening pass
over the whole LDE domain (bj_deep_quotient_d, prover.rs:2523-2706), timed with HIP events on the
stream they run on.  Nothing existing computes these on the device, so the yardstick is a
device-to-device copy of the same number of bytes in the same run on the same GPU.

* evaluate_at: algorithmic bytes per launch = C*n*8 (coset 0 of every column) + 2*n*8 (weights).
* deep_quotient: C*N*8 (every column over the domain, N = n*D) + 2*N*8 (the codeword written).
* copy: hipMemcpyAsync device to device of as many bytes as the kernel reads from the columns; its
  rate counts the bytes read plus the bytes written (2 x the bytes copied).

Both kernels are HBM-bound by design (two Goldilocks products per element read), so "frac" is
achieved bytes/s over the 8 TB/s peak and "vs_copy" the same rate over the copy's.

usage: python tools/deep_bench.py [log_n=22] [n_cols=256] [log_d=2]   (prints one JSON line)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

HBM_PEAK_GBS = 8000.0


def timed(torch, fn, reps):
    st = torch.cuda.current_stream()
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    import numpy as np
    import torch
    from boojum_amd import deep
    from boojum_amd._lib import call
    from boojum_amd.field import P, stream_of, to_device
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    log_d = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    if not torch.cuda.is_available():
        raise SystemExit("deep_bench needs a GPU")
    n, log_domain = 1 << log_n, log_n + log_d
    domain = 1 << log_domain
    lde = torch.empty((n_cols, domain), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", lde.data_ptr(), n_cols, domain, log_domain, 7, 0, stream_of(lde))
    rng = np.random.default_rng(1)
    z = tuple(int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64))
    k = tuple(int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64))
    gammas = to_device(rng.integers(0, P, size=2 * n_cols, dtype=np.uint64))
    w0, w1 = deep.precompute_for_barycentric_evaluation_in_extension(n, 7, z)
    out = torch.empty((n_cols, 2), dtype=torch.int64, device="cuda")
    d0 = torch.empty((domain,), dtype=torch.int64, device="cuda")
    d1 = torch.empty_like(d0)
    st = stream_of(lde)

    def evaluate():
        call("bj_evaluate_at_d", lde.data_ptr(), n_cols, domain, log_n, w0.data_ptr(), w1.data_ptr(), out.data_ptr(),
             st)

    def quotient():
        call("bj_deep_quotient_d", lde.data_ptr(), n_cols, domain, gammas.data_ptr(), k[0], k[1], z[0], z[1],
             log_domain, 0, domain, d0.data_ptr(), d1.data_ptr(), 0, st)

    t_weights = timed(torch, lambda: deep.precompute_for_barycentric_evaluation_in_extension(n, 7, z), 10)
    t_eval = timed(torch, evaluate, 100)
    t_quot = timed(torch, quotient, 30)
    eval_bytes = n_cols * n * 8 + 2 * n * 8
    quot_bytes = n_cols * domain * 8 + 2 * domain * 8
    # the yardstick: device-to-device copies of the bytes each kernel reads from the columns
    dst = torch.empty_like(lde)
    src1, dst1 = lde.reshape(-1), dst.reshape(-1)
    eval_words = n_cols * n

    t_copy_eval = timed(torch, lambda: dst1[:eval_words].copy_(src1[:eval_words]), 100)
    t_copy_quot = timed(torch, lambda: dst1.copy_(src1), 20)
    copy_eval_gbs = 2 * eval_words * 8 / t_copy_eval / 1e9
    copy_quot_gbs = 2 * src1.numel() * 8 / t_copy_quot / 1e9

    def row(t, nbytes, copy_t, copy_gbs, copied):
        gbs = nbytes / t / 1e9
        return {"ms": t * 1e3, "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": gbs / HBM_PEAK_GBS, "alg_bytes_per_launch": nbytes,
                "copy": {"bytes_copied": copied, "ms": copy_t * 1e3, "read_plus_write_gbs": copy_gbs},
                "vs_copy": gbs / copy_gbs}

    line = {
        "shape": "%d columns x 2^%d rows, D = %d (domain 2^%d)" % (n_cols, log_n, 1 << log_d, log_domain),
        "device": torch.cuda.get_device_name(0),
        "barycentric_weights": {"ms": t_weights * 1e3},
        "evaluate_at": row(t_eval, eval_bytes, t_copy_eval, copy_eval_gbs, eval_words * 8),
        "deep_quotient": row(t_quot, quot_bytes, t_copy_quot, copy_quot_gbs, src1.numel() * 8),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
