"""Where a secret may reach an address or a branch in the device source: the committed list that tests/test_secret_taint.py holds
MemorySanitizer's reports against.  Everything else is a failure, and so is an entry that no case reaches.

kind: `address` (a load or store whose address derives from a secret) or `branch`.  function: the innermost function outside the
C model of the instructions (tests/host_emul/valu_model.h, coop_wave.h).  licence: the sentence of DESIGN.md section 8 that allows
it.  There is no `branch` entry: no operation with a secret input branches on anything derived from it."""
import collections

Entry = collections.namedtuple("Entry", "kind function reason licence")

ROWS = "Without a context the walk is as exposed as the reference's: rows are fetched by secret index"
PEER_ROWS = "there the secret selects rows and nothing else (every column adds a row, row 0 included"

ALLOWED = (
    Entry("address", "lds_load_pa_signed", "one lane's row of a signed 8 x 32 comb table in LDS, chosen by a column byte of the scalar", ROWS),
    Entry("address", "wb_load_pa_signed", "one lane's row of the wide comb in device memory (base point, or the one remembered peer's), chosen by a 13-bit column",
          ROWS),
    Entry("address", "row_limb", "the per-wave form of lds_load_pa_signed: each lane reads its limb of the chosen 8 x 32 comb row", ROWS),
    Entry("address", "packed_limb", "the per-wave form of wb_load_pa_signed: each lane unpacks its limb from the chosen wide-comb row", ROWS),
    Entry("address", "row_field_fetch", "the quad form of wb_load_pa_signed: each of four lanes reads its field of the chosen wide-comb row", ROWS),
    Entry("address", "peer_ctx_row", "the row of a peer context's table that a column of the secret selects", PEER_ROWS),
)


def allows(kind: str, function: str) -> bool:
    return any(e.kind == kind and e.function == function for e in ALLOWED)
