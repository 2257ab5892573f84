#!/usr/bin/env python3
"""prove -> record-in-HBM, eight routes alternating in one process on one MI355X:
  host    prove_proof + verifier.stwo_record + upload          | prove_many(workers) + the same conversion
  device  prove_record (ss_p_finish_dev, ss_p_decommit_record) | prove_records(workers)
  devtx   prove_record(transcript="device"): the transcript before the FRI commit on the GPU as well
          (include/ss_prover_transcript.h)                     | prove_records(workers, transcript="device")
  fritail devtx with fri_tail=True: the FRI layers that fit in one workgroup committed by one launch
          (include/ss_prover_fri.h)                            | prove_records(workers, transcript="device", fri_tail=True)
  gridpow devtx with grid_pow=True: the proof of work ground by a grid of workgroups over the whole device
          (include/ss_prover_pow.h; span 2^(pow_bits + 8))      | prove_records(workers, transcript="device", grid_pow=True)
  small   the whole batch in ONE launch, a workgroup per proof (include/ss_prover_small.h; shapes within GpuProver.small_limits())
          prove_records([0], one_launch=True)                  | prove_records(range(proofs), one_launch=True)
  minimal prove_minimal_record (ss_p_decommit_minimal): the MINIMAL record, planned and gathered on the device
                                                               | prove_minimal_records(workers): + ss_p_minimal_pack_dev
  minhost the minimal record without that kernel: prove_record, download, verifier.stwo_minimise_record, upload
          (the queries it needs are taken as known: replayed before the clock starts)   | prove_records + the same
All end with the record(s) resident and the device synchronised; host / device / devtx / fritail / gridpow / small must hold the
same words, and so must minimal / minhost.
`python tools/prover_record_bench.py [trace_log] [reps] [proofs] [workers] [n_cols] [pow_bits] [routes] [log_blowup] [n_queries]`
(wide256: 14 15 48 4 256); `routes` = a comma-separated choice of the names above (default: all but small), e.g.
`devtx,gridpow` at 20 bits, where devtx's search outgrows ss_p_finish_dev's span and falls back to the host, or
`devtx,fritail,small` at 9 6 4096 (proof.json's shape) and 3 6 4096 4 4 5 devtx,fritail,small 1 1 (proof_test.json's)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stark_symphony_amd import prover, verifier  # noqa: E402

trace_log = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
n_many = int(sys.argv[3]) if len(sys.argv) > 3 else 48
workers = int(sys.argv[4]) if len(sys.argv) > 4 else 4
n_cols = int(sys.argv[5]) if len(sys.argv) > 5 else 4
pow_bits = int(sys.argv[6]) if len(sys.argv) > 6 else 5
chosen = sys.argv[7].split(",") if len(sys.argv) > 7 else None
log_blowup = int(sys.argv[8]) if len(sys.argv) > 8 else 4
n_queries = int(sys.argv[9]) if len(sys.argv) > 9 else 16
kw = dict(n_cols=n_cols, trace_log=trace_log, log_blowup=log_blowup, n_queries=n_queries, pow_bits=pow_bits, hash="sha256")
gp = prover.GpuProver(verifier.Verifier(0))
torch = gp.torch


def upload(proofs):
    rec = torch.from_numpy(np.stack([verifier.stwo_record(p) for p in proofs]).view(np.int32)).to(gp.dev)
    torch.cuda.synchronize(gp.dev)
    return rec


cfg = gp.config(**kw)
queries = []  # of seed i, for the minhost route
for seed in range(n_many if chosen is None or "minhost" in chosen else 0):  # (chosen is None: every route but small)
    gp.prove_proof(seed=seed, **kw)
    queries.append(list(gp.queries))


def minimise_upload(rows):
    host = rows.cpu().numpy().view(np.uint32)
    mins = [verifier.stwo_minimise_record(cfg, host[i], queries[i]) for i in range(host.shape[0])]
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([m.size for m in mins])]).astype(np.int64)).to(gp.dev)
    flat = torch.from_numpy(np.concatenate(mins).view(np.int32)).to(gp.dev)
    torch.cuda.synchronize(gp.dev)
    return flat, offs


def timed(fn):
    torch.cuda.synchronize(gp.dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(gp.dev)
    return time.perf_counter() - t0, out


routes = {
    "host_one": lambda: upload([gp.prove_proof(seed=0, **kw)])[0],
    "device_one": lambda: gp.prove_record(seed=0, **kw),
    "devtx_one": lambda: gp.prove_record(seed=0, transcript="device", **kw),
    "fritail_one": lambda: gp.prove_record(seed=0, transcript="device", fri_tail=True, **kw),
    "gridpow_one": lambda: gp.prove_record(seed=0, transcript="device", grid_pow=True, **kw),
    "small_one": lambda: gp.prove_records([0], one_launch=True, **kw)[0],
    "minimal_one": lambda: gp.prove_minimal_record(seed=0, **kw),
    "minhost_one": lambda: minimise_upload(gp.prove_record(seed=0, **kw)[None])[0],
    "host_many": lambda: upload(gp.prove_many(range(n_many), workers=workers, **kw)),
    "device_many": lambda: gp.prove_records(range(n_many), workers=workers, **kw),
    "devtx_many": lambda: gp.prove_records(range(n_many), workers=workers, transcript="device", **kw),
    "fritail_many": lambda: gp.prove_records(range(n_many), workers=workers, transcript="device", fri_tail=True, **kw),
    "gridpow_many": lambda: gp.prove_records(range(n_many), workers=workers, transcript="device", grid_pow=True, **kw),
    "small_many": lambda: gp.prove_records(range(n_many), one_launch=True, **kw),
    "minimal_many": lambda: gp.prove_minimal_records(range(n_many), workers=workers, **kw),
    "minhost_many": lambda: minimise_upload(gp.prove_records(range(n_many), workers=workers, **kw)),
}
if chosen is None:  # (small serves small shapes only: by name)
    chosen = [k for k in ("host", "device", "devtx", "fritail", "gridpow", "minimal", "minhost")]
routes = {k: v for k, v in routes.items() if k.rsplit("_", 1)[0] in chosen}


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)


times = {k: [] for k in routes}
for r in range(reps + 1):  # round 0 warms every route (allocator pools, worker streams, code objects)
    outs = {}
    for name, fn in routes.items():
        if name.endswith("many") and r > (reps + 2) // 3:
            continue
        dt, outs[name] = timed(fn)
        if r:
            times[name].append(dt / (n_many if name.endswith("many") else 1))
    for group in (("host", "device", "devtx", "fritail", "gridpow", "small"), ("minimal", "minhost")):
        for suffix in ("_one", "_many"):
            got = [outs[g + suffix] for g in group if g + suffix in outs]
            assert all(same(got[0], x) for x in got[1:]), (group, suffix)
result = {k: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "runs": len(v)}
          for k, v in times.items()}
print(json.dumps({"metric": "prove -> resident record, 2^%d x %d, blowup %d, Q=%d, per proof" % (trace_log, n_cols, 1 << log_blowup, n_queries),
                  "pow_bits": pow_bits, "record_words": next((v.numel() for k, v in outs.items() if k.endswith("_one") and not k.startswith("min")), None),
                  "minimal_words_seed0": outs["minimal_one"].numel() if "minimal_one" in outs else None,
                  "proofs_in_many": n_many, "workers": workers, "routes": result}))
