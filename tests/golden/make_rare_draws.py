#!/usr/bin/env python3
"""Search channel states whose channel_draw_qm31 takes its rare branch, and write them to rare_draws.json.

channel_draw_qm31 (stwo-verifier/src/channel.simf:115-140) hashes digest || be4(counter), advances the counter, and throws
the draw away when one of the first four big-endian words is >= 2^32 - 2.  Per draw that happens with probability 2^-29, so
no proof, fixture or known-answer literal ever gets there; this script finds, by plain search in hashlib,

  unit      (digest, counter) states whose first draw holds 0xFFFFFFFD (accepted, reduces to P - 1), 0xFFFFFFFE or
            0xFFFFFFFF (both redrawn) among its first four words; digest = H(b"rare-draw-%d" % i), counter 0 or 3
  verifier  one word of roots[2], and one word of the first FRI root, of the smallest numpy-prover proof for which the
            draw that follows the root's mix (t, resp. the first fold alpha) is redrawn
  fri_tail  a channel state and a FRI layer of 2 and of 4 QM31 values whose last word is such that the draw after the mix
            of the layer's Merkle root is redrawn

for SHA-256 and Blake2s.  Every entry is confirmed by the restatement below before the file is written, and an incomplete
set is never written.  No test runs the search (it is some 10^10 hashes); `--check` re-confirms the committed file in
seconds.  Only the Blake2s proof the verifier entries start from needs tools/stwo_prover.py (numpy); all else is hashlib.

    python tests/golden/make_rare_draws.py [--jobs N]     search and write rare_draws.json
    python tests/golden/make_rare_draws.py --check        confirm every entry of the committed file
"""
import argparse
import collections
import hashlib
import json
import multiprocessing
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rare_draws.json")
P = (1 << 31) - 1
HASHES = {"sha256": hashlib.sha256, "blake2s": lambda b=b"": hashlib.blake2s(b, digest_size=32)}
UNIT_WORDS = (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF)
UNIT_COUNTERS = (0, 3)
SMALLEST = dict(n_cols=4, trace_log=3, log_blowup=1, n_queries=1, pow_bits=5)
VERIFIER_FIELDS = (("roots[2]", 5), ("fri_roots[0]", 2))  # (field, index of the word that is replaced)
TAIL_LOGS = (1, 2)
TAIL_WORD = 3      # the word of the layer's last value that is varied (below P: the layer holds field elements)
CHUNK = 1 << 21


# ------------------------------------------------------------------------------------------ the restatement
def words(b):
    return [int.from_bytes(b[4 * i:4 * i + 4], "big") for i in range(len(b) // 4)]


def be(ws):
    return b"".join(int(w).to_bytes(4, "big") for w in ws)


def draw_qm31(H, digest, counter):
    """-> (four field elements, counter afterwards, attempts, first four words of the first attempt)"""
    attempts, first = 0, None
    while True:
        w = words(H(digest + counter.to_bytes(4, "big")).digest())[:4]
        counter += 1
        attempts += 1
        first = first or w
        if all(x < (1 << 32) - 2 for x in w):
            return [x % P for x in w], counter, attempts, first


def rare(out, least=0xFFFFFFFE):
    """the first of the first four words of a draw's hash that is >= least, or None"""
    if b"\xff\xff\xff" not in out[:16]:
        return None
    for w in words(out[:16]):
        if w >= least:
            return w
    return None


def smallest_proof(hash):
    if hash == "sha256":
        return json.load(open(os.path.join(HERE, "stwo_proof_test.json")))
    sys.path.insert(0, os.path.join(HERE, "..", "..", "tools"))
    import stwo_prover
    return stwo_prover.prove(hash=hash, **SMALLEST)


def flat(v):
    return [v[0][0], v[0][1], v[1][0], v[1][1]]


def digest_before(H, proof, field):
    """the channel's digest just before `field` is mixed (draws leave the digest alone)"""
    d = bytes(32)
    for root in proof["commitments"][:2]:
        d = H(d + bytes(root)).digest()
    if field == "roots[2]":
        return d
    d = H(d + bytes(proof["commitments"][2])).digest()
    oods = [flat(col[0]) for tree in proof["sampled_values"][1:] for col in tree]
    return H(d + b"".join(be(v) for v in oods)).digest()


def field_of(proof, field):
    return bytes(proof["commitments"][2] if field == "roots[2]" else proof["fri_proof"]["first_layer"]["commitment"])


def tail_root(H, layer):
    level = [H(be(v)).digest() for v in layer]
    while len(level) > 1:
        level = [H(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
    return level[0]


def tail_start(hash, log_n):
    """the state and the layer before the search: hashes of fixed strings"""
    H = HASHES[hash]
    state = words(H(b"rare-tail-state-%d" % log_n).digest()) + [3]
    layer = [[w % P for w in words(H(b"rare-tail-layer-%d-%d" % (log_n, i)).digest())[:4]] for i in range(1 << log_n)]
    return state, layer


def confirm(doc):
    """every entry against the restatement; raises on the first that does not take its branch"""
    seen = set()
    for e in doc["unit"]:
        H = HASHES[e["hash"]]
        digest = H(b"rare-draw-%d" % e["seed"]).digest()
        assert digest.hex() == e["digest"], e
        _, after, attempts, first = draw_qm31(H, digest, e["counter"])
        assert e["word"] in first and rare(be(first), 0xFFFFFFFD) == e["word"], e
        assert attempts == (1 if e["word"] == 0xFFFFFFFD else 2) and after == e["counter"] + attempts, e
        seen.add((e["hash"], e["word"]))
        seen.add((e["hash"], "counter", e["counter"] != 0))
    for hash in HASHES:
        assert all((hash, w) in seen for w in UNIT_WORDS) and (hash, "counter", False) in seen and (hash, "counter", True) in seen, hash
    proofs = {}
    for e in doc["verifier"]:
        H = HASHES[e["hash"]]
        proof = proofs.setdefault(e["hash"], smallest_proof(e["hash"]))
        root = words(field_of(proof, e["field"]))
        assert root[e["word"]] != e["value"], e
        root[e["word"]] = e["value"]
        _, after, attempts, _ = draw_qm31(H, H(digest_before(H, proof, e["field"]) + be(root)).digest(), 0)
        assert attempts == 2 and after == 2, e
        seen.add((e["hash"], e["field"]))
    for e in doc["fri_tail"]:
        H = HASHES[e["hash"]]
        assert len(e["state"]) == 9 and len(e["layer"]) == 1 << e["log_n"] and all(0 <= w < P for v in e["layer"] for w in v), e
        start = tail_start(e["hash"], e["log_n"])
        assert e["state"] == start[0] and e["layer"][:-1] == start[1][:-1] and e["layer"][-1][:TAIL_WORD] == start[1][-1][:TAIL_WORD], e
        _, after, attempts, _ = draw_qm31(H, H(be(e["state"][:8]) + tail_root(H, e["layer"])).digest(), 0)
        assert attempts == 2 and after == 2, e
        seen.add((e["hash"], "tail", e["log_n"]))
    for hash in HASHES:
        assert all((hash, f) in seen for f, _ in VERIFIER_FIELDS) and all((hash, "tail", n) in seen for n in TAIL_LOGS), hash
    return len(doc["unit"]), len(doc["verifier"]), len(doc["fri_tail"])


# ------------------------------------------------------------------------------------------------ the search
def unit_chunk(job):
    hash, lo = job
    H, hits, counters = HASHES[hash], [], [(c, c.to_bytes(4, "big")) for c in UNIT_COUNTERS]
    for i in range(lo, lo + CHUNK):
        d = H(b"rare-draw-%d" % i).digest()
        for c, c4 in counters:
            out = H(d + c4).digest()
            if b"\xff\xff\xff" in out[:16] and rare(out, 0xFFFFFFFD) is not None:  # (the cheap test first: 2^31 times)
                hits.append((i, c, rare(out, 0xFFFFFFFD)))
    return hits


def chain_chunk(job):
    """hash, lo, limit, bytes before the varied word, bytes after it, then the left siblings up to the root and the
    digest the root is mixed into (both empty for a root that is itself the message) -> the first word that redraws"""
    hash, lo, limit, head, tail, siblings, digest = job
    H, zero = HASHES[hash], bytes(4)
    for w in range(lo, min(lo + CHUNK, limit)):
        d = H(head + w.to_bytes(4, "big") + tail).digest()
        for s in siblings:
            d = H(s + d).digest()
        if digest:
            d = H(digest + d).digest()
        out = H(d + zero).digest()
        if b"\xff\xff\xff" in out[:16] and rare(out) is not None:
            return w
    return None


def search(pool, width, worker, jobs, done):
    """ordered, so the result does not depend on the number of processes -> (candidates chunks, seconds)"""
    t0, n, window = time.time(), 0, collections.deque()
    for job in jobs:
        window.append(pool.apply_async(worker, (job,)))
        if len(window) < 4 * width:
            continue
        n += 1
        if done(window.popleft().get()):
            return n, time.time() - t0
    while window:
        n += 1
        if done(window.popleft().get()):
            break
    return n, time.time() - t0


def jobs_from(make):
    lo = 0
    while True:
        job = make(lo)
        if job is None:
            return
        yield job
        lo += CHUNK


def generate(n_jobs):
    doc = {"about": "channel states whose draw_qm31 takes a rare branch; written by make_rare_draws.py, confirmed by its --check",
           "unit": [], "verifier": [], "fri_tail": [], "search": {}}
    t_all = time.time()

    def note(key, candidates, seconds):
        doc["search"][key] = {"candidates": candidates, "seconds": round(seconds, 1)}
        print("%-28s %12d candidates %8.1f s" % (key, candidates, seconds), file=sys.stderr, flush=True)
    for hash in HASHES:
        H = HASHES[hash]
        # -- unit states: the first state of every (word, counter) pair seen until all three words and both counters are there
        found = {}

        def unit_done(hits):
            for i, c, w in hits:
                found.setdefault((w, c), i)
            return {w for w, _ in found} == set(UNIT_WORDS) and {c for _, c in found} == set(UNIT_COUNTERS)
        with multiprocessing.Pool(n_jobs) as pool:
            n, secs = search(pool, n_jobs, unit_chunk, jobs_from(lambda lo: (hash, lo)), unit_done)
        note("unit/" + hash, n * CHUNK * len(UNIT_COUNTERS), secs)
        for (w, c), i in sorted(found.items()):
            doc["unit"].append({"hash": hash, "seed": i, "digest": H(b"rare-draw-%d" % i).digest().hex(), "counter": c, "word": w})
        # -- verifier records
        proof = smallest_proof(hash)
        for field, k in VERIFIER_FIELDS:
            root, got = field_of(proof, field), []
            head, tail = digest_before(H, proof, field) + root[:4 * k], root[4 * k + 4:]
            with multiprocessing.Pool(n_jobs) as pool:
                n, secs = search(pool, n_jobs, chain_chunk,
                                 jobs_from(lambda lo: (hash, lo, 1 << 32, head, tail, [], b"") if lo < 1 << 32 else None),
                                 lambda w: w is not None and not got.append(w))
            if not got:
                raise SystemExit("%s %s: no word of 2^32 redraws" % (hash, field))
            note("verifier/%s/%s" % (hash, field), (n - 1) * CHUNK + got[0] % CHUNK + 1, secs)
            doc["verifier"].append({"hash": hash, "field": field, "word": k, "value": got[0]})
        # -- FRI-tail inputs
        for log_n in TAIL_LOGS:
            state, layer = tail_start(hash, log_n)
            level, siblings = [H(be(v)).digest() for v in layer], []
            while len(level) > 1:
                siblings.append(level[-2])
                level = [H(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
            head, got = be(layer[-1][:TAIL_WORD]), []
            with multiprocessing.Pool(n_jobs) as pool:
                n, secs = search(pool, n_jobs, chain_chunk,
                                 jobs_from(lambda lo: (hash, lo, P, head, be(layer[-1][TAIL_WORD + 1:]), siblings, be(state[:8])) if lo < P else None),
                                 lambda w: w is not None and not got.append(w))
            if not got:
                raise SystemExit("%s tail %d: no word below P redraws" % (hash, log_n))
            note("fri_tail/%s/log%d" % (hash, log_n), (n - 1) * CHUNK + got[0] % CHUNK + 1, secs)
            layer[-1][TAIL_WORD] = got[0]
            doc["fri_tail"].append({"hash": hash, "log_n": log_n, "state": state, "layer": layer})
    doc["search"]["total"] = {"candidates": sum(v["candidates"] for v in doc["search"].values()),
                              "seconds": round(time.time() - t_all, 1), "processes": n_jobs}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="confirm the committed rare_draws.json and exit")
    ap.add_argument("--jobs", type=int, default=os.cpu_count())
    args = ap.parse_args()
    if args.check:
        print("rare_draws.json: %d unit states, %d verifier records, %d FRI-tail inputs confirmed" % confirm(json.load(open(OUT))))
        return
    doc = generate(args.jobs)
    confirm(doc)  # (raises before anything is written)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s" % OUT, file=sys.stderr)


if __name__ == "__main__":
    main()
