"""The redraw of channel_draw_qm31 (stwo-verifier/src/channel.simf:115-140) on the host: a draw whose first four words hold one
>= 2^32 - 2 is thrown away and taken again with the counter one higher.  Per draw that happens with probability 2^-29, so no
proof, fixture or known-answer literal takes the branch; tests/golden/rare_draws.json (make_rare_draws.py) holds states that do.

The reference of every test here and in test_gpu_rare_draws.py is the restatement below -- H(digest || be4(counter)), the
four-word check, % P, in hashlib and Python integers -- and never prover._Channel, stwo_prover.Channel, formats.stwo_queries or
the oracle: those are the host copies of the draw, and they are under test.  Every test first asserts on the restatement
alone that the branch it is about is taken."""
import dataclasses
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stwo_prover  # noqa: E402

import stark_symphony_amd as ss  # noqa: E402
from stark_symphony_amd import formats, prover, verifier  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
P = (1 << 31) - 1
HASHES = {"sha256": hashlib.sha256, "blake2s": lambda b: hashlib.blake2s(b, digest_size=32)}
SMALLEST = dict(n_cols=4, trace_log=3, log_blowup=1, n_queries=1, pow_bits=5)
with open(os.path.join(GOLDEN, "rare_draws.json")) as _f:
    RARE = json.load(_f)
UNIT = [pytest.param(e, id="%s-%08x-ctr%d" % (e["hash"], e["word"], e["counter"])) for e in RARE["unit"]]
RECORDS = [pytest.param(e, id="%s-%s" % (e["hash"], e["field"])) for e in RARE["verifier"]]
TAILS = [pytest.param(e, id="%s-log%d" % (e["hash"], e["log_n"])) for e in RARE["fri_tail"]]


# ------------------------------------------------------------------------------------------------- the restatement
def be(ws) -> bytes:
    return b"".join(int(w).to_bytes(4, "big") for w in np.asarray(ws).reshape(-1).tolist())


def words(b: bytes):
    return [int.from_bytes(b[4 * i:4 * i + 4], "big") for i in range(len(b) // 4)]


def draw(H, digest: bytes, counter: int):
    """channel_draw_qm31 -> (the four field elements, the counter afterwards, attempts, the first attempt's four words)"""
    first = None
    for attempt in range(1, 257):
        w = words(H(digest + counter.to_bytes(4, "big")).digest())[:4]
        counter += 1
        first = first or w
        if w[0] < 2 ** 32 - 2 and w[1] < 2 ** 32 - 2 and w[2] < 2 ** 32 - 2 and w[3] < 2 ** 32 - 2:
            return tuple(x % P for x in w), counter, attempt, first
    raise AssertionError("256 attempts")


def cmul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def qmul(x, y):  # (A + B u)(C + D u), u^2 = 2 + i
    a, b, c, d = x[:2], x[2:], y[:2], y[2:]
    ac, bd, ad, bc = cmul(a, c), cmul(b, d), cmul(a, d), cmul(b, c)
    r = cmul(bd, (2, 1))
    return ((ac[0] + r[0]) % P, (ac[1] + r[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P)


def qinv(x):  # (A - B u) / (A^2 - (2 + i) B^2)
    a, b = x[:2], x[2:]
    r = cmul(cmul(b, b), (2, 1))
    den = ((cmul(a, a)[0] - r[0]) % P, (cmul(a, a)[1] - r[1]) % P)
    n = pow(den[0] * den[0] + den[1] * den[1], P - 2, P)
    inv = (den[0] * n % P, -den[1] * n % P)
    return cmul(a, inv) + cmul(((-b[0]) % P, (-b[1]) % P), inv)


def point_of(t):
    """channel_draw_qm31_point (channel.simf:143-151): ((1 - t^2) / (1 + t^2), 2 t / (1 + t^2)) -> 8 words"""
    t2 = qmul(t, t)
    inv = qinv(((1 + t2[0]) % P,) + t2[1:])
    return qmul(((1 - t2[0]) % P,) + tuple((-v) % P for v in t2[1:]), inv) + qmul(tuple(2 * v % P for v in t), inv)


def transcript(p, nonce=None):
    """The verifier's Fiat-Shamir chain over proof `p` (verifier.simf:32-58) -> dict: attempts of every draw in order
    (cp_alpha, t, deep_alpha, one per FRI layer), oods_point[8], fold_alphas, pow_value (LE64 of the last 8 bytes of the
    digest after the nonce's mix), queries."""
    H = HASHES[p.cfg.hash]
    st = {"d": bytes(32), "c": 0, "attempts": [], "first": []}

    def mix(b):
        st["d"], st["c"] = H(st["d"] + b).digest(), 0

    def draw_qm31():
        v, st["c"], n, first = draw(H, st["d"], st["c"])
        st["attempts"].append(n)
        st["first"].append(first)
        return v
    mix(bytes(p.roots[0])); mix(bytes(p.roots[1])); draw_qm31(); mix(bytes(p.roots[2]))
    t = draw_qm31()
    mix(be(p.oods_trace) + be(p.oods_cp))
    draw_qm31()
    alphas = []
    for r in p.fri_roots:
        mix(bytes(r))
        alphas.append(list(draw_qm31()))
    mix(be(p.last_layer))
    before_nonce = st["d"]
    mix(int(p.pow_nonce if nonce is None else nonce).to_bytes(8, "big"))
    value, queries = int.from_bytes(st["d"][24:], "little"), []
    while len(queries) < p.cfg.n_queries:
        queries += [w & ((1 << p.cfg.lde_log) - 1) for w in words(H(st["d"] + st["c"].to_bytes(4, "big")).digest())]
        st["c"] += 1
    return {"attempts": st["attempts"], "first_words": st["first"], "oods_point": list(point_of(t)), "fold_alphas": alphas, "pow_value": value,
            "queries": queries[:p.cfg.n_queries], "digest_before_nonce": before_nonce}


@functools.lru_cache(maxsize=None)
def smallest_proof(hash):
    """the numpy prover's proof of the smallest shape (SHA-256: stwo_proof_test.json, which it reproduces byte for byte)"""
    if hash == "sha256":
        with open(os.path.join(GOLDEN, "stwo_proof_test.json")) as f:
            return ss.stwo_from_json(json.load(f))
    return ss.stwo_from_json(stwo_prover.prove(hash=hash, **SMALLEST), trace_log=SMALLEST["trace_log"])


def record_proof(e):
    """the smallest proof with the one word of rare_draws.json's verifier entry `e` replaced"""
    p = smallest_proof(e["hash"]).copy()
    row = p.roots[2] if e["field"] == "roots[2]" else p.fri_roots[0]
    assert e["field"] in ("roots[2]", "fri_roots[0]")
    row[4 * e["word"]:4 * e["word"] + 4] = np.frombuffer(int(e["value"]).to_bytes(4, "big"), dtype=np.uint8)
    return p


def tail_first_words(e):
    """the first four words of the draw behind the mix of layer 0's root, for a fri_tail entry of rare_draws.json"""
    H = HASHES[e["hash"]]
    level = [H(be(v)).digest() for v in e["layer"]]
    while len(level) > 1:
        level = [H(level[2 * i] + level[2 * i + 1]).digest() for i in range(len(level) // 2)]
    return draw(H, H(be(e["state"][:8]) + level[0]).digest(), 0)[3]


def redrawn_ordinal(e):
    return 1 if e["field"] == "roots[2]" else 3  # draws in order: cp_alpha, t, deep_alpha, fold alpha 0, ...


def expected_record_status(e, mode, status):
    """The stage order (verifier.simf:32-58; csrc/ss_stwo.hip) decides what a verifier record must report.  The redraw itself
    fails nothing.  A changed word of roots[2] changes t, so the OODS point moves off the sampled values: the first failing
    assert is stage II's `cp_eval == sampled`, stwo_code(2, 0, 0, 3), in both modes.  A changed word of the first FRI root
    leaves stages I-II as they were and changes the digest the nonce is mixed into: stage IV fails with stwo_code(4, 0, 0, 0)
    when the restated pow value misses the target (31 cases of 32), otherwise a stage behind it does (the root no longer
    heads the layer's tree)."""
    if e["field"] == "roots[2]":
        return status == verifier.stwo_code(2, 0, 0, 3)
    p = record_proof(e)
    if transcript(p)["pow_value"] >= p.cfg.pow_target:
        return status == verifier.stwo_code(4, 0, 0, 0)
    return status >> 24 > 4


@dataclasses.dataclass(frozen=True)
class TargetConfig(formats.StwoConfig):
    """a StwoConfig whose 64-bit target is the caller's own word (ss_stwo_cfg.pow_target is one), not 2^(64 - pow_bits) - 1"""
    target: int = 0

    @property
    def pow_target(self) -> int:
        return self.target


def with_target(p, target):
    q = p.copy()
    q.cfg = TargetConfig(**dataclasses.asdict(p.cfg), target=target)
    return q


def pow_cases(p):
    """-> [(target, expected status of the valid proof p in FIXTURE mode)]: check_proof_of_work (pow.simf:22-36) asserts
    value < target on all 64 bits, so the status is stwo_code(4, 0, 0, 0) exactly when value >= target, by arithmetic.
    The value itself and its successor; bit 32 moved up and down; the low word cleared, and carried into the high word."""
    v = transcript(p)["pow_value"]
    assert 1 << 32 <= v < p.cfg.pow_target
    targets = [v, v + 1, v + (1 << 32), v - (1 << 32), v & ~0xFFFFFFFF, (v | 0xFFFFFFFF) + 1]
    return [(t, 0 if v < t else verifier.stwo_code(4, 0, 0, 0)) for t in targets]


def high_nonce(p):
    """the first nonce >= 2^32 that meets p's target behind p's transcript"""
    H, digest = HASHES[p.cfg.hash], transcript(p)["digest_before_nonce"]
    return next(n for n in range(1 << 32, (1 << 32) + (1 << 16))
                if int.from_bytes(H(digest + n.to_bytes(8, "big")).digest()[24:], "little") < p.cfg.pow_target)


# ----------------------------------------------------------------------------------------------------------- tests
def test_the_fixture_covers_every_branch_for_both_hashes():
    for hash in HASHES:
        have = {(e["word"], e["counter"] != 0) for e in RARE["unit"] if e["hash"] == hash}
        assert {w for w, _ in have} == {0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF} and {c for _, c in have} == {False, True}
        assert {e["field"] for e in RARE["verifier"] if e["hash"] == hash} == {"roots[2]", "fri_roots[0]"}
        assert {e["log_n"] for e in RARE["fri_tail"] if e["hash"] == hash} == {1, 2}
    # 0xFFFFFFFE is the boundary: the least word that is redrawn, and the one a `<=` for `<` or a limit one too high accepts.
    # Every unit state set has it (above); of the verifier records and the FRI-tail inputs at least one per site must.
    for field in ("roots[2]", "fri_roots[0]"):
        assert any(0xFFFFFFFE in transcript(record_proof(e))["first_words"][redrawn_ordinal(e)] for e in RARE["verifier"] if e["field"] == field)
    assert any(0xFFFFFFFE in tail_first_words(e) for e in RARE["fri_tail"])


@pytest.mark.parametrize("e", UNIT)
def test_host_draws_equal_the_restatement_on_unit_states(e):
    H, digest, counter = HASHES[e["hash"]], bytes.fromhex(e["digest"]), e["counter"]
    value, after, attempts, first = draw(H, digest, counter)
    # the branch, on the restatement alone
    assert e["word"] in first and attempts == (1 if e["word"] == 0xFFFFFFFD else 2) and after == counter + attempts
    if e["word"] == 0xFFFFFFFD:
        assert value[first.index(e["word"])] == P - 1
    assert O.channel_draw_qm31(digest, counter, e["hash"]) == (0, value, after)
    ch = prover._Channel(prover.HASHES[e["hash"]])
    ch.digest, ch.counter = digest, counter
    assert (tuple(ch.draw_qm31()), ch.counter, ch.digest) == (value, after, digest)
    stwo_prover._H = stwo_prover.HASHES[e["hash"]]
    try:
        ch = stwo_prover.Channel()
        ch.digest, ch.counter = digest, counter
        assert (tuple(int(x) for x in ch.draw_qm31()), ch.counter, ch.digest) == (value, after, digest)
    finally:
        stwo_prover._H = hashlib.sha256


@pytest.mark.parametrize("e", RECORDS)
def test_oracle_verifies_the_verifier_records_past_the_redraw(e):
    p = record_proof(e)
    ref, honest = transcript(p), transcript(smallest_proof(e["hash"]))
    want = [1] * len(ref["attempts"])
    want[redrawn_ordinal(e)] = 2
    assert ref["attempts"] == want and honest["attempts"] == [1] * len(want)  # the branch, on the restatement alone
    assert formats.stwo_queries(p) == ref["queries"]  # (formats.py's own copy of the chain)
    for mode in (O.MODE_FIXTURE, O.MODE_LITERAL):
        status, tr = O.stwo_verify(p, mode, trace=True)
        assert status >> 24 != 1 and expected_record_status(e, mode, status), hex(status)
        assert list(tr.oods_point.x.t()) + list(tr.oods_point.y.t()) == ref["oods_point"]
        assert [list(tr.fold_alpha[l].t()) for l in range(p.cfg.n_layers + 1)] == ref["fold_alphas"]
        assert list(tr.queries[:p.cfg.n_queries]) == ref["queries"]


@pytest.mark.parametrize("which", ["small", "prod", "small-blake2s"])
def test_oracle_compares_all_64_bits_of_the_pow_value_strictly(stwo_small, stwo_prod, which):
    base = {"small": stwo_small, "prod": stwo_prod}.get(which) or smallest_proof("blake2s")
    cases = pow_cases(base)
    assert [want for _, want in cases] == [verifier.stwo_code(4, 0, 0, 0), 0, 0, verifier.stwo_code(4, 0, 0, 0), verifier.stwo_code(4, 0, 0, 0), 0]
    for target, want in cases:
        assert O.stwo_verify(with_target(base, target), O.MODE_FIXTURE) == want, hex(target)


@pytest.mark.parametrize("hash", ["sha256", "blake2s"])
def test_oracle_mixes_a_nonce_with_a_high_word_in_full(hash):
    p = smallest_proof(hash).copy()
    p.pow_nonce = high_nonce(p)
    ref = transcript(p)
    assert p.pow_nonce >> 32 == 1 and ref["pow_value"] < p.cfg.pow_target
    status, tr = O.stwo_verify(p, O.MODE_FIXTURE, trace=True)
    assert status != verifier.stwo_code(4, 0, 0, 0) and list(tr.queries[:p.cfg.n_queries]) == ref["queries"]
    assert formats.stwo_queries(p) == ref["queries"]
