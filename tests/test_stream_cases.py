"""What tests/test_gpu_streams.py's assertions rest on, checked with the oracle and the Python models alone (no GPU): the three rule
sets agree on the verification rows, every set has accepted and rejected rows, the edge peers are what they claim, and the two path
models give the hook values the issue of each scenario states."""
import numpy as np

import check_zip215_model as czm
import one_peer_cases as opc
import stream_cases as sc
import strict_cases
from vectors import L, P

ZIP215_SAMPLE = 64           # the big-integer ZIP-215 model takes ~20 ms a row: the first rows of a one-key block (every kind of
                             # flip, 7 rows apart) and as many seeded ones; the rotation's distinct rows are modelled one and all


def three_rules(sig, pk, msg, plain, rows):
    """the strict rule on every row, the ZIP-215 model on `rows`: both the oracle's verdict"""
    assert np.array_equal(strict_cases.strict_rule(sig, pk, plain), plain)
    assert np.array_equal(czm.model_verdicts(sig[rows], pk[rows], msg[rows]), plain[rows])


def test_one_key_rows_have_one_verdict_under_all_three_rules(oracle):
    for pub, sig, msg, ok in sc.one_key_sets(oracle):
        n = len(sig)
        assert n == sc.BLOCK and sc.A_ROWS % n == 0 and sc.ONE_KEY_WIDE % n == 0 and sc.SMALL <= n
        rows = np.r_[0:ZIP215_SAMPLE, np.random.default_rng(0x57A1).choice(np.arange(ZIP215_SAMPLE, n), ZIP215_SAMPLE, replace=False)]
        three_rules(sig, np.repeat(pub, n, axis=0), msg, ok, rows)
        want = np.ones(n, np.int32)
        want[0::7] = want[2::7] = want[4::7] = 0
        assert np.array_equal(ok, want)                    # exactly the flipped rows are rejected
        assert all(int.from_bytes(s[32:].tobytes(), "little") < L for s in sig[:ZIP215_SAMPLE])
        assert 0 < ok[:sc.SMALL].sum() < sc.SMALL           # the small calls see both verdicts too
    k0, k1 = (s[0].tobytes() for s in sc.one_key_sets(oracle))
    assert k0 != k1


def test_rotation_rows_have_one_verdict_under_all_three_rules(oracle):
    d = sc.rotation_set(oracle)
    vsig, vpk, vmsg = d["v_distinct"]
    plain = oracle.ed25519_verify(vsig, vpk, vmsg)
    three_rules(vsig, vpk, vmsg, plain, np.arange(sc.ROT_DISTINCT))
    for m in (sc.ROT_SMALL, sc.ROT_LARGE):
        assert 0 < d["v_ok"][:m].sum() < m
        assert np.array_equal(d["v_ok"][:m], sc.tile(plain, m))
        assert (d["valid_rows"] < m).sum() > m // 2
    # the garbage keys: rejected under every rule, some of them because the key does not decode (the plain call's slow list)
    g = d["g_rows"]
    assert g[0] < sc.ROT_SMALL and len(g) == sc.ROT_LARGE // sc.GARBAGE_EVERY
    assert not d["g_ok"][g].any()
    assert not czm.model_verdicts(d["v_sig"][g], d["g_pk"][g], d["v_msg"][g]).any()
    assert not strict_cases.strict_rule(d["v_sig"][g], d["g_pk"][g], d["g_ok"][g]).any()
    rest = np.setdiff1d(np.arange(sc.ROT_LARGE), g)
    assert np.array_equal(d["g_ok"][rest], d["v_ok"][rest])
    assert 0 < sc.slow_rows(d, sc.ROT_LARGE) < len(g)
    assert len(set(d["idx"].reshape(-1)[:sc.ROT_SMALL])) == sc.ROT_KEYS     # every context is used at both sizes
    # signing and key derivation: what the oracle says for the keys the rows name
    assert np.array_equal(oracle.ed25519_verify(d["sig"][:64], d["pub"][d["idx"].reshape(-1)[:64]], d["msg"][:64]), np.ones(64, np.int32))
    assert set(d["c_flags"][:sc.ROT_SMALL]) == set(d["c_flags"]) and len(set(d["c_flags"])) > 4


def test_edge_peers_are_what_they_claim(oracle):
    sk, peers = sc.one_peer_sets(oracle)
    u = {name: int.from_bytes(pk.tobytes(), "little") for name, (pk, _, _) in peers.items()}
    assert opc.on_curve(u["p0"]) and opc.on_curve(u["p1"]) and u["p0"] != u["p1"]
    assert opc.eligible(u["p0"]) and opc.eligible(u["p1"])
    assert not opc.on_curve(u["twist"])
    assert u["minus_one"] == P - 1 and not opc.eligible(u["minus_one"])
    for name in peers:
        assert sc.peer_eligible(name) == opc.eligible(u[name])
    # u = p - 1 has order 4 (on the twist): every clamped secret is a multiple of 8, so every shared key is 32 zero bytes
    assert not peers["minus_one"][1].any()
    for name in ("p0", "p1", "twist"):
        shared, clamped = peers[name][1], peers[name][2]
        assert shared.any(axis=1).all()
        for i in (0, 1, sc.SMALL - 1, sc.BLOCK - 1):        # the oracle against the big-integer ladder
            assert shared[i].tobytes() == opc.shared(peers[name][0].tobytes(), sk[i].tobytes())
            assert int.from_bytes(clamped[i].tobytes(), "little") == opc.clamp(int.from_bytes(sk[i].tobytes(), "little"))
    assert len({peers[name][1][:8].tobytes() for name in peers}) == 4


def test_path_models_give_the_stated_hook_values():
    calls = lambda table, order: [table[c] for c, _ in order]  # noqa: E731
    assert sc.check_paths(calls(sc.VERIFY_CALLS, sc.VERIFY_ORDERS["handover"])) == [1, 1, 0, 1]       # A, B, C, D
    assert sc.check_paths(calls(sc.VERIFY_CALLS, sc.VERIFY_ORDERS["swapped"])) == [1, 1, 0, 1]
    assert sc.check_paths(calls(sc.VERIFY_CALLS, sc.VERIFY_ORDERS["one_stream"])) == [1, 1, 0, 1]
    assert sc.check_paths(calls(sc.VERIFY_CALLS, sc.VERIFY_ORDERS["b_first"])) == [1, 1, 1, 0]        # B, A, C, D
    assert sc.peer_paths(calls(sc.PEER_CALLS, sc.PEER_ORDERS["handover"])) == [1, 1, 0, 0, 0, 1]      # A, B, T, M, C, D
    assert sc.peer_paths(calls(sc.PEER_CALLS, sc.PEER_ORDERS["b_first"])) == [1, 1, 0, 0, 1, 0]       # B, A, T, M, C, D
    assert sc.peer_paths(calls(sc.PEER_CALLS, sc.PEER_ORDERS["third_stream"])) == [1, 1, 0, 0, 0, 1]
    for name in ("handover", "swapped", "b_first"):         # only A and B open a stream: the calls that answer "ladder" come behind them
        first = {}
        for c, s_ in sc.PEER_ORDERS[name]:
            first.setdefault(s_, c)
        assert sorted(first.values()) == ["A", "B"]
    assert sc.check_paths([(0, sc.SMALL), (0, sc.COOP_MAX)]) == [0, 0]                                # nothing kept, per-wave size
    for order in list(sc.VERIFY_ORDERS.values()) + list(sc.PEER_ORDERS.values()):
        assert {s for _, s in order} <= {0, 1, 2}
    assert sc.VERIFY_CALLS["A"][1] >= 1 << 17 and sc.VERIFY_CALLS["B"][1] == 1 << 16 and sc.PEER_CALLS["B"][1] >= sc.ONE_PEER_WIDE and sc.PEER_CALLS["A"][1] >= 1 << 17
    assert {s for _, _, s in sc.BOTH_ORDER} == {0, 1, 2}
    assert [c for k, c, _ in sc.BOTH_ORDER if k == "verify"] == list("ABCD") and [c for k, c, _ in sc.BOTH_ORDER if k == "peer"] == list("ABTMCD")
