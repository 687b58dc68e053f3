"""tests/vrf_model.py against RFC 9381's three examples for ECVRF-EDWARDS25519-SHA512-ELL2 (appendix B.3: public key, proof and
output of each; H, U and V of the first), and the properties its case set relies on: every honest row verifies and hashes to the
same beta, every rejection row is rejected for the reason its label gives, the proofs crafted for the keys of small order satisfy
both equations (they verify with validate_key off) and fall to validate_key alone, and the key of mixed order is accepted exactly
when [c]T8 vanishes."""
import pytest

import vrf_model as m
from vectors import L


@pytest.mark.parametrize("i", range(3))
def test_rfc_example(i):
    e = m.EXAMPLES[i]
    sk, alpha = bytes.fromhex(e["sk"]), bytes.fromhex(e["alpha"])
    assert m.public_key(sk).hex() == e["pk"]
    parts = m.prove_parts(m.private_key(sk), alpha)
    for name in ("H", "U", "V"):
        if name in e:
            assert parts[name].hex() == e[name], name
    assert parts["pi"].hex() == e["pi"]
    assert m.proof_to_hash(parts["pi"]) == (bytes.fromhex(e["beta"]), 1)
    assert m.verify(bytes.fromhex(e["pk"]), parts["pi"], alpha) == (bytes.fromhex(e["beta"]), 1)


def test_the_dst_and_the_lengths():
    assert len(m.DST) == 40 and m.DST[-1] == 4
    assert len(m.ALPHA_LENGTHS) == len(set(m.ALPHA_LENGTHS)) == 12


@pytest.mark.parametrize("alpha_len", m.ALPHA_LENGTHS)
def test_honest_rows_verify(alpha_len):
    h = m.honest(alpha_len)
    for pk, alpha, pi, beta in zip(h["pk"], h["alpha"], h["pi"], h["beta"]):
        assert m.verify(pk.tobytes(), pi.tobytes(), alpha.tobytes()) == (beta.tobytes(), 1)
        assert m.proof_to_hash(pi.tobytes()) == (beta.tobytes(), 1)
        assert int.from_bytes(pi.tobytes()[48:], "little") < L


def test_rejection_rows():
    r = m.rejections()
    accepted = {lab for lab, ok in zip(r["labels"], r["ok"]) if ok}
    assert accepted == {"honest", "honest, second key", "a key of mixed order, c a multiple of 8"}
    for lab, pi, ok, beta, ok_hash, beta_hash in zip(r["labels"], r["pi"], r["ok"], r["beta"], r["ok_hash"], r["beta_hash"]):
        if ok:
            assert ok_hash and beta.tobytes() == beta_hash.tobytes() != m.ZERO_BETA, lab
        else:
            assert beta.tobytes() == m.ZERO_BETA, lab
        # ProofToHash looks at the proof alone: it rejects what does not decode and nothing else (a flipped bit of Gamma may land
        # on the curve or off it; the rows named here cannot decode, the negated Gamma must)
        undecodable = m.decode_proof(pi.tobytes()) is None
        if lab.startswith(("s + L", "s = L", "s with bit 255", "Gamma off", "Gamma not canonical")):
            assert undecodable, lab
        if lab == "Gamma negated" or "key" in lab or "alpha" in lab or "of c" in lab:
            assert not undecodable, lab
        assert bool(ok_hash) == (not undecodable), lab
        assert (beta_hash.tobytes() == m.ZERO_BETA) == undecodable, lab


def test_small_order_keys_fall_to_validate_key_alone():
    r = m.rejections()
    rows = [(lab, pk.tobytes(), pi.tobytes(), a.tobytes()) for lab, pk, pi, a in zip(r["labels"], r["pk"], r["pi"], r["alpha"])
            if "crafted" in lab]
    assert len(rows) == 8 and len({k for _, k, _, _ in rows}) == 8
    for lab, pk, pi, alpha in rows:
        assert m.verify(pk, pi, alpha, validate_key=False)[1] == 1, lab
        assert m.verify(pk, pi, alpha, validate_key=True) == (m.ZERO_BETA, 0), lab
    assert sorted(order for _, order in m.small_order_keys()) == [1, 2, 4, 4, 8, 8, 8, 8]


def test_mixed_order_rows():
    import key_model
    priv, alpha, pi = m.mixed_order_privs()
    for p, a, q, want in zip(priv, alpha, pi, (1, 0)):
        assert key_model.classify(p.tobytes()[32:]) == key_model.DECODES | key_model.CANONICAL
        assert m.verify(p.tobytes()[32:], q.tobytes(), a.tobytes())[1] == want
        c = int.from_bytes(q.tobytes()[32:48], "little")
        assert (c % 8 == 0) == bool(want)
