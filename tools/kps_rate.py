"""Time kmers-per-sample (mf_kps.hip) on one resident synthetic cohort, next to kmers-samples-counter on the same tables (the yardstick:
the same union pass over the same entries, read out once).

The cohort is tools/stats3_rate.py's: --n samples of --reads reads each, counted by the library at k = 31.  One warm-up, then --steps
repeats, device-synchronised wall time, the best is reported; the per-kernel times ([launches, total ms]) are the library's HIP-event
timers (option profile = 1) over one more repeat.
  --what kps        mf_kmers_per_sample_tables(tables, max_bad 0, percent) for every --perc; then, on each result, the device formatter
                    (k_kps_widths + scan + k_kps_format + the download of the text: mf_kps_row_text) per row against a plain single-thread
                    host loop that formats the same row (C, compiled here with the system's cc; CPython's str / join as well for rows of
                    up to 5 M values)
  --what nsamples   mf_kmers_samples_count_tables(tables, max_bad 0); --root names another checkout of this project whose built library is
                    measured instead (the parent commit's)

    python tools/kps_rate.py --what kps --perc 20 50
    python tools/kps_rate.py --what nsamples --root ../parent
"""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=("kps", "nsamples"), required=True)
ap.add_argument("--n", type=int, default=32)
ap.add_argument("--reads", type=int, default=2_000_000)
ap.add_argument("--read-len", type=int, default=100)
ap.add_argument("-k", type=int, default=31)
ap.add_argument("--perc", type=int, nargs="+", default=[20, 50])
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from metafast_amd import lib as L  # noqa: E402

SEEDS = (0x41414141, 0x42424242, 0x43434343)

HOST_LOOP_C = r"""
#include <stdint.h>
/* "\t" + decimal per value, one thread: returns the bytes written */
uint64_t format_row(const uint16_t *row, uint64_t m, char *out) {
    char *o = out;
    for (uint64_t i = 0; i < m; i++) {
        unsigned v = row[i];
        char d[5]; int n = 0;
        do { d[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        *o++ = '\t';
        while (n) *o++ = d[--n];
    }
    return (uint64_t)(o - out);
}
"""


def synth_table(ctx, j, group, n_reads, k, rl):
    n1 = n_reads * 4 // 5
    n2 = n_reads - n1
    bases = torch.zeros(n_reads * rl + 64, dtype=torch.uint8, device="cuda")
    offs = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    ctx.synth_reads_device(0x5354415453, j, 0, n1, rl, 1_000_000, bases.data_ptr(), offs.data_ptr())
    ctx.synth_reads_device(SEEDS[group], 0, j * n2, n2, rl, 100_000, bases.data_ptr() + n1 * rl, offs[n1:].data_ptr())
    offs[n1:] += n1 * rl
    t = ctx.count_device(bases.data_ptr(), offs.data_ptr(), n_reads, n_reads * rl, k, 0)
    torch.cuda.synchronize()
    return t


def timed(fn, steps):
    fn()                                                       # warm-up (arena, code objects)
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def kernels(ctx, fn):
    ctx.set_option("profile", 1)                               # one more repeat under the event timers (they are off for the wall times)
    ctx.reset_timers()
    fn()
    torch.cuda.synchronize()
    ctx.set_option("profile", 0)
    return {name: [n, round(ms, 3)] for name, (n, ms, mx) in sorted(ctx.kernel_report().items()) if n}


def host_loop():
    """the C loop as a callable (row uint16[M]) -> bytes, or None where there is no compiler"""
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        return None
    d = tempfile.mkdtemp()
    src, so = os.path.join(d, "f.c"), os.path.join(d, "f.so")
    open(src, "w").write(HOST_LOOP_C)
    if subprocess.run([cc, "-O2", "-shared", "-fPIC", src, "-o", so]).returncode != 0:
        return None
    f = ctypes.CDLL(so).format_row
    f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]

    def run(row):
        out = np.empty(len(row) * 6, np.uint8)
        return out[:f(row.ctypes.data, len(row), out.ctypes.data)].tobytes()
    return run


class _DeviceRow:
    """sample j's row of the resident matrix, for torch to copy (the values as int16: same bits)"""

    def __init__(self, ptr, m, j):
        self.__cuda_array_interface__ = dict(shape=(m,), typestr="<i2", data=(ptr + 2 * m * j, False), version=2)


def formatter(ctx, r, perc, c_loop):
    """row 1 of the result: device formatter + download against the host loops"""
    m = r.shape()[1]
    if not m:
        return dict(perc=perc, values=0)
    row = torch.as_tensor(_DeviceRow(r.device_view()[2], m, 1), device="cuda").cpu().numpy().view(np.uint16).copy()
    text, dev = timed(lambda: r.row_text(1), args.steps)
    fmt = dict(perc=perc, values=m, text_bytes=len(text), device_format_and_download_s=[round(t, 5) for t in dev],
               device_best_s=round(min(dev), 5), device_kernel_ms=kernels(ctx, lambda: r.row_text(1)))
    if c_loop is not None:
        t_c, host = timed(lambda: c_loop(row), args.steps)
        assert t_c == text
        fmt.update(host_c_loop_s=[round(t, 5) for t in host], host_c_best_s=round(min(host), 5))
    if m <= 5_000_000:
        t_py, py = timed(lambda: ("\t" + "\t".join(map(str, row.tolist()))).encode(), args.steps)
        assert t_py == text
        fmt.update(host_cpython_join_s=[round(t, 5) for t in py], host_cpython_best_s=round(min(py), 5))
    return fmt


def main():
    ctx = L.Context(0, stream=torch.cuda.current_stream())
    tabs = [synth_table(ctx, j, j * 3 // args.n, args.reads, args.k, args.read_len) for j in range(args.n)]
    res = dict(what=args.what, root=os.path.abspath(args.root), samples=args.n, reads_per_sample=args.reads, k=args.k, steps=args.steps,
               entries=sum(len(t) for t in tabs))
    if args.what == "nsamples":
        def fn():
            t = ctx.kmers_samples_count(tabs, 0)
            n = len(t)
            t.close()
            return n
        n, times = timed(fn, args.steps)
        res.update(n_kmers=n, wall_s=[round(t, 4) for t in times], wall_s_best=round(min(times), 4), kernel_ms=kernels(ctx, fn))
        print(json.dumps(res))
        return
    c_loop = host_loop()
    for perc in args.perc:
        def fn():
            r = ctx.kmers_per_sample(tabs, percent=perc)
            shape = r.shape()
            r.close()
            return shape
        shape, times = timed(fn, args.steps)
        res["perc_%d" % perc] = dict(selected_kmers=shape[1], matrix_bytes=shape[0] * shape[1] * 2, wall_s=[round(t, 4) for t in times],
                                     wall_s_best=round(min(times), 4), kernel_ms=kernels(ctx, fn))
        r = ctx.kmers_per_sample(tabs, percent=perc)
        res["perc_%d" % perc]["formatter"] = formatter(ctx, r, perc, c_loop)
        r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
