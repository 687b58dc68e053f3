"""The big-integer model of the scalar calls (tests/scalar_model.py) against itself and against fixed vectors: what every other
scalar test compares the device code with must be right first."""
import numpy as np

import scalar_model as model
from scalar_model import L

# (call, the inputs' little-endian bytes one after the other, the canonical result): inputs are SHA-512 halves of fixed strings, the
# edges L - 1, 2^256 - 1 and 2^512 - 1, and values whose answer is known without any arithmetic (1/2 = (L + 1)/2, -1 = L - 1,
# 1 - 0 = 1, (L - 1)^2 = 1, L 2^256 = 0)
VECTORS = (
    ("reduce", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad039186408270aa99200510f99da599878fe4dfd065c68a563e35bd428cbf03f3d",
     "b8f3cb666808c89a312695baef0af572c60427730d0a6c99345da2bd7d7f640b"),
    ("reduce", "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
     "000f9c44e31106a447938568a71b0ed065bef517d273ecce3d9a307c1b419903"),
    ("reduce", "0000000000000000000000000000000000000000000000000000000000000000edd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010",
     "0000000000000000000000000000000000000000000000000000000000000000"),
    ("add", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad05a33af5d760af67b4fa2e86c72f28065dee171fd98ed1da873805f3c83ba9cca",
     "c83a85c1f442d9b065144bec1fca6772ecce53696abb13ea03ceb5b9d9fbb60a"),
    ("sub", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad05a33af5d760af67b4fa2e86c72f28065dee171fd98ed1da873805f3c83ba9cca",
     "3986281a9bdbb852b520a8fcf84b2cb1310b706e38e0d7991ccdf640d3867d05"),
    ("mul", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad05a33af5d760af67b4fa2e86c72f28065dee171fd98ed1da873805f3c83ba9cca",
     "ec0aa7d8ee19083b049463fb3b063fa1b938c5da8595d666ff5451d83dc7a909"),
    ("mul", "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",
     "a28c56e32e7552a6122e79c77b57ed6b68bef517d273ecce3d9a307c1b419903"),
    ("negate", "0100000000000000000000000000000000000000000000000000000000000000",
     "ecd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010"),
    ("negate", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad0",
     "63dd999d5f855202b4d0f97fc16b840df1121e942e320abe6fb2a982a9bee50f"),
    ("complement", "0000000000000000000000000000000000000000000000000000000000000000",
     "0100000000000000000000000000000000000000000000000000000000000000"),
    ("complement", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad0",
     "64dd999d5f855202b4d0f97fc16b840df1121e942e320abe6fb2a982a9bee50f"),
    ("muladd", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad05a33af5d760af67b4fa2e86c72f28065dee171fd98ed1da873805f3c83ba9cca39186408270aa99200510f99da599878fe4dfd065c68a563e35bd428cbf03f3d",
     "71d3336dac97676dab7194089c785bc6b786c2e1e1fd7bcae2b0250109b8e906"),
    ("invert", "0200000000000000000000000000000000000000000000000000000000000000",
     "f7e97a2e8d31092c6bce7b51ef7c6f0a00000000000000000000000000000008"),
    ("invert", "93b9d77711e6aece04c390696b3ead1610ede16bd1cdf541904d567d56411ad0",
     "01ff36e121fd69c728d47dc20a540fd6f744213b07fe109975b8a95fcc712203"),
    ("invert", "ecd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010",
     "ecd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010"),
)


def test_the_order():
    assert L.to_bytes(32, "little").hex() == "edd3f55c1a631258d69cf7a2def9de1400000000000000000000000000000010"
    assert pow(2, L - 1, L) == 1 and pow(3, L - 1, L) == 1 and 15 * L + 1 < 2**256 < 16 * L


def test_fixed_vectors():
    for call, inputs, want in VECTORS:
        raw = bytes.fromhex(inputs)
        width = 64 if call == "reduce" else 32
        args = [int.from_bytes(raw[i:i + width], "little") for i in range(0, len(raw), width)]
        got = getattr(model, call)(*args)
        if call == "invert":
            assert got[1] == 1
            got = got[0]
        assert got.to_bytes(32, "little").hex() == want, (call, inputs)


def test_the_model_against_itself():
    xs = model.values32()
    assert len(xs) > 4096 and len(set(xs)) > 4096
    for x in xs:
        r, ok = model.invert(x)
        assert ok == (x % L != 0) and 0 <= r < L
        assert model.mul(x, r) == ok, hex(x)
        assert model.negate(model.negate(x)) == x % L
        assert model.complement(model.complement(x)) == x % L
        assert model.add(x, model.negate(x)) == 0 and model.sub(x, x) == 0
        assert model.is_canonical(x) == (model.reduce(x) == x)
    assert model.invert(0) == (0, 0) and model.invert(L) == (0, 0) and model.invert(15 * L) == (0, 0), "zero is judged after reduction"
    assert model.invert(1) == (1, 1) and model.invert(L + 1) == (1, 1)


def test_the_case_set():
    c = model.case_set()
    n = len(model.values32())
    assert all(c[k].shape == (n, 32) for k in ("x", "y", "z", "add", "sub", "mul", "negate", "complement", "muladd", "recip"))
    assert c["w"].shape == (len(model.values64()), 64) and c["reduce"].shape == (len(model.values64()), 32)
    assert c["ok"].shape == (n,) and 0 < (c["ok"] == 0).sum() < 32 and 0 < (c["canonical"] == 0).sum() < n
    x, y, z = (model.from_rows(c[k]) for k in ("x", "y", "z"))
    for i in (0, 3, 4, 5, 77, n - 1):
        assert model.from_rows(c["muladd"][i:i + 1])[0] == (x[i] * y[i] + z[i]) % L
    assert not c["x"].flags.writeable
    assert np.array_equal(model.cycled(c["x"], n + 3)[n:], c["x"][:3])
    for w, r in zip(model.values64(), model.from_rows(c["reduce"])):
        assert r == w % L
