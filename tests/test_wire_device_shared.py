"""The three wire dialects and the reply compaction on ONE context, one call
after another: the ingests' per-call words share one device allocation, grown
by the largest call and carved anew by each, so every call here follows one of
another dialect or another size.  Every call's outputs are compared with the
host decoder's through the dialects' own test helpers (guard bytes included),
never with the device path itself.
"""
import numpy as np
import pytest

import test_wire_device as Y
import test_wire_device_calvin as V
import test_wire_device_tpcc as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402


def test_the_dialects_take_turns_on_one_context():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    eng = dvcc.CCEngine(dvcc.NO_WAIT, 8192, 1 << 17)
    try:
        rng = np.random.default_rng(31)
        ycsb = Y._good_row(rng, 5)
        Y.run_and_check(eng, ycsb, next_txn=3)
        # grows the words; two scan chunks
        pos = V.run_and_check(eng, V._good_row(rng, V.CHUNK + 1), expect=(V.C.END, (V.CHUNK + 1, 0)))
        assert pos.n_txn == V.CHUNK + 1
        Y.run_and_check(eng, ycsb, next_txn=3)
        P.run_and_check(eng, P._good_row(rng, 1))
        ing, dep, host, ep = Y._reply_epoch(eng, Y.REPLY_TILE + 1)
        c = (np.arange(Y.REPLY_TILE + 1) % 3 != 1).astype(np.uint8)
        assert ing.respond(dep, torch.from_numpy(c).cuda()) == host.respond(ep, c)
        V.run_and_check(eng, V._good_row(rng, 5), prior=(2, 7, 0, 4), expect=(V.C.END, (5, 0)))
    finally:
        eng.close()
