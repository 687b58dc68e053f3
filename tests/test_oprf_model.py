"""The big-integer model of the OPRF / VOPRF calls (tests/oprf_model.py) pinned to published vectors -- not to the code under test --
and checked against itself, and the coverage of the case set the host-emulation and GPU tests share.

Where the vectors come from.  The mode-0 vector is RFC 9497 A.1.1 as tests/test_h2c_model.py holds it (imported from there).  The
three mode-1 vectors (oprf_model.VECTORS) are the values the issue that asked for these calls states: computed with this repository's
own models following RFC 9497 sections 2.2.1 and 2.2.2, and reported there to agree with the RFC's A.1.2.1 to A.1.2.3 in keys,
elements and proofs as its author remembered them -- the RFC's text was not at hand when they were pinned, so they are a record of
the construction at that point (seed a3 x 32, info "test key", the RFC's blinds), not an independent transcription."""
import h2c_model
import oprf_model as model
import ristretto_model
import test_h2c_model as a11
from vectors import L


def test_the_mode_1_key_pair():
    sks = h2c_model.oprf_derive_key_pair(model.VOPRF_SEED, model.VOPRF_INFO, 1)
    assert sks.hex() == model.VOPRF_SKS
    assert model.base_mult(int.from_bytes(sks, "little")).hex() == model.VOPRF_PKS


def test_the_mode_0_vector():
    blinded, ok = model.blind(a11.OPRF_INPUT, bytes.fromhex(a11.OPRF_BLIND), 0)
    assert ok == 1 and blinded.hex() == a11.OPRF_BLINDED
    evaluated, ok, _ = model.evaluate_row(bytes.fromhex(a11.OPRF_SKS), blinded)
    assert ok == 1 and evaluated.hex() == a11.OPRF_EVALUATION
    out, ok, _ = model.finalize(a11.OPRF_INPUT, bytes.fromhex(a11.OPRF_BLIND), evaluated)
    assert ok == 1 and out.hex() == a11.OPRF_OUTPUT


def test_the_mode_1_vectors():
    sks, pks = bytes.fromhex(model.VOPRF_SKS), bytes.fromhex(model.VOPRF_PKS)
    for v in model.VECTORS:
        n = len(v["inputs"])
        blinded = [model.blind(i, bytes.fromhex(b), 1) for i, b in zip(v["inputs"], v["blinds"])]
        assert [b[0].hex() for b in blinded] == list(v["blinded"]) and all(b[1] for b in blinded)
        rows = [b[0] for b in blinded]
        evaluated, proofs, ok, req_ok = model.voprf_blind_evaluate(sks, [bytes.fromhex(v["r"])], rows, [0, n])
        assert [e.hex() for e in evaluated] == list(v["evaluated"]) and ok == [1] * n and req_ok == [1]
        assert proofs[0].hex() == v["proof"]
        assert model.voprf_verify(pks, rows, evaluated, proofs, [0, n]) == [1]
        outs = [model.finalize(i, bytes.fromhex(b), e) for i, b, e in zip(v["inputs"], v["blinds"], evaluated)]
        assert [o[0].hex() for o in outs] == list(v["outputs"])
    assert model.VECTORS[2]["outputs"] == model.VECTORS[0]["outputs"] + model.VECTORS[1]["outputs"]


def test_the_proof_is_the_schnorr_identity():
    """s B + c pkS = r B and s M + c Z = r M for the model's own proof, with the composites summed term by term (no known logarithms)"""
    c = model.request_case(False)
    off = [int(x) for x in c["offsets"]]
    j = c["sizes"].index(3)
    rows = range(off[j], off[j + 1])
    cs, ds = [bytes(c["blinded"][i]) for i in rows], [bytes(c["evaluated"][i]) for i in rows]
    fast = model.composites(c["pks"], cs, ds, [c["logs"][i] for i in rows], model.KEY)
    slow = model.composites(c["pks"], cs, ds)
    assert model._enc(fast[0]) == model._enc(slow[0]) and model._enc(fast[1]) == model._enc(slow[1])
    assert model.verify_proof(c["pks"], cs, ds, bytes(c["proof"][j])) == 1


def test_input_lengths_sit_on_both_sides_of_every_edge():
    assert model.INPUT_LENGTHS == (0, 1, 17, 66, 67, 68, 83, 84, 85, 300)
    assert [(n + model.HASH_TO_GROUP_DST_LEN + 4) % 128 for n in model.INPUT_LENGTHS[3:9]] == list(h2c_model.EDGE_RESIDUES)
    assert [(n + model.FINALIZE_TAIL) % 128 for n in model.INPUT_LENGTHS[3:9]] == list(h2c_model.EDGE_RESIDUES)
    # Finalize's padding: 0x80 and sixteen length bytes behind len + 44 bytes -- a second block from 68 on, a third at 300
    assert [(n + 44 + 17 + 127) // 128 for n in (66, 67, 68)] == [1, 1, 2] and (300 + 44 + 17 + 127) // 128 == 3


def test_request_sizes_and_rejections_are_what_the_labels_say():
    assert model.REQUEST_SIZES == (1, 2, 3, 63, 64, 65, 255, 256, 257)
    assert sorted(model.request_case(True)["sizes"]) == sorted(model.REQUEST_SIZES) and model.request_case(True)["sizes"] != model.REQUEST_SIZES
    labels = [c["label"] for c in model.server_rejections()]
    for must in ("identity row", "skS 0", "skS L", "proof_rand 0", "proof_rand L"):
        assert must in labels
    assert sum(lab.startswith("undecodable row") for lab in labels) == len(ristretto_model.FIXED_REJECTS)
    by = {c["label"]: c["want"] for c in model.server_rejections()}
    assert by["proof_rand 0"]["req_ok"] == [1, 1, 0, 1] and not by["proof_rand 0"]["proof"][2].any() and by["proof_rand 0"]["ok"] == [1] * 10
    assert by["skS L"]["req_ok"] == [0] * 4 and by["skS L"]["ok"] == [0] * 10
    labels = [c["label"] for c in model.verify_rejections()]
    for must in ("c + L", "s + L", "a flipped bit of c", "a flipped bit of s", "a flipped bit of an evaluated row", "a wrong pkS",
                 "an undecodable pkS", "two rows of a request swapped", "the last row of a request given to the next"):
        assert must in labels
    assert {r[2].split(":")[0] for r in model.row_rejections()} == {"undecodable", "identity", "blind 0", "blind L", "valid"}


def test_owners_of_well_formed_offsets_are_the_requests():
    off = model.request_offsets((3, 1, 4))
    assert model.owners(off, 3, 8) == [0, 0, 0, 1, 2, 2, 2, 2]
    assert model.owners([0, 5, 3, 8], 3, 8) == [0, 0, 0, 2, 2, 2, 2, 2]         # any array gives one definite answer: request 0 has lost rows 3 and 4
    assert model.owners([0, 3, 3, 8], 3, 8)[3:] == [2] * 5
    assert model.owners([0, 70000], 1, 70000) == [model.NO_OWNER] * 70000


def test_scalars_are_read_mod_l():
    inp = b"abc"
    b = model._scalar("mod L")
    assert model.blind(inp, model._le(b), 0) == model.blind(inp, model._le(b + L), 0)
    assert model.blind(inp, model._le(L), 1) == (model.ZERO32, 0)
