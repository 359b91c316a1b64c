"""The batch log of the Python pipes (sdrdaemon_amd.engine._BatchLog) on its own: no library, no GPU.  The log mirrors what the
library's batch ring holds -- which batches are launched, which one is being filled, and the nb_fec / log2interp each launched
batch keeps -- so that the collects can size and shape their buffers; these are the rules the pipes rely on."""
import numpy as np

from sdrdaemon_amd.engine import _BatchLog


def test_uniform_batches_launch_after_blocks_fills():
    log = _BatchLog()
    log.reset(blocks=3)
    log.block("uniform", 1000, 4)
    log.block("uniform", 500, 4)
    assert log.head(4) == (None, 4) and log.filling.size == 1500  # (two fills: nothing launched)
    log.block("uniform", 7, 8)
    rec, cfg = log.head(32)
    assert (rec.kind, rec.size, rec.cfg, cfg) == ("uniform", 1507, 8, 8)  # (the summed size; the nb_fec of the third fill)
    assert log.filling is None and len(log.batches) == 1


def test_wait_flushes_the_filling_batch():
    log = _BatchLog(blocks=4)
    assert log.head(16, "uniform") == (None, 16) and not log.batches and log.filling is None  # (nothing to flush: unchanged)
    log.block("uniform", 300, 4)
    assert log.head(8) == (None, 8) and log.filling is not None  # (wait = False: the batch goes on filling)
    assert log.head(8, "ragged") == (None, 8) and log.filling is not None  # (a collect of another kind sends nothing out)
    rec, cfg = log.head(8, "uniform")
    assert (rec.kind, rec.size, rec.cfg, cfg) == ("uniform", 300, 8, 8)  # (launched under the setting of the flush)
    assert log.filling is None and log.batches == [rec]
    assert log.head(32, "uniform") == (rec, 8)  # (a launched batch is not launched again)
    log.block("uniform", 100, 4)
    assert log.head(32, "uniform") == (rec, 8) and log.filling.size == 100  # (a batch in front: the filling one stays)


def test_ragged_counts_add_per_stream():
    log = _BatchLog(blocks=2)
    log.block("ragged", np.array([5, 0, 9]), 4)
    log.block("ragged", np.array([1, 2, 3]), 6)
    rec, cfg = log.head(32)
    assert rec.kind == "ragged" and rec.size.tolist() == [6, 2, 12] and rec.most == 12 and cfg == 6
    log.block("ragged", np.zeros(0, np.int64), 6)
    assert log.filling.most == 0  # (a bank of no streams)


def test_datagram_batches_are_one_record_per_submit_and_pop_in_order():
    log = _BatchLog(blocks=5)  # (`blocks` is about blocks of samples: a datagram batch is launched by its one submit)
    for cfg in (4, 8, 16):
        log.batch("datagram", None, cfg)
    assert [b.cfg for b in log.batches] == [4, 8, 16] and log.filling is None
    rec, cfg = log.head(32)
    assert (rec.kind, rec.most, cfg) == ("datagram", 0, 4)
    assert log.head(32)[1] == 4 and len(log.batches) == 3  # (the call that learns the counts, rc -1, reads and does not pop)
    log.pop()
    assert log.head(32)[1] == 8
    log.pop()
    log.pop()
    assert log.head(32) == (None, 32)
    log.pop()  # (a batch the log was not told of -- submitted through the C entry -- : nothing to forget)
    assert log.head(32) == (None, 32)


def test_kind_at_the_head():
    log = _BatchLog()
    log.block("ragged", np.array([3, 4]), 4)
    log.batch("datagram", None, 8)
    assert log.head(32)[0].kind == "ragged"
    log.pop()
    assert log.head(32)[0].kind == "datagram"


def test_reset_empties_the_log_and_takes_the_new_blocks():
    log = _BatchLog(blocks=2)
    log.block("uniform", 10, 4)
    log.block("uniform", 10, 4)
    log.block("uniform", 10, 4)
    log.pop()
    assert log.last == 20 and log.filling is not None
    log.reset(blocks=3)
    assert (log.blocks, log.batches, log.filling, log.last) == (3, [], None, 0)
    log.block("uniform", 1, 4)
    log.block("uniform", 1, 4)
    assert not log.batches
    log.block("uniform", 1, 4)
    assert len(log.batches) == 1


def test_a_fresh_log_is_the_default_ring_of_one_block_batches():
    log = _BatchLog()
    assert (log.blocks, log.batches, log.filling, log.last, log.sample_room()) == (1, [], None, 0, 0)
    for n in (11, 22, 33, 44):  # (depth 4: the library refuses a fifth submit, and a refused submit is not logged)
        log.block("uniform", n, 4)
    assert [b.size for b in log.batches] == [11, 22, 33, 44] and log.filling is None


def test_the_previous_batch_size_follows_the_last_popped_record():
    log = _BatchLog(blocks=2)
    log.block("uniform", 5000, 4)
    log.block("uniform", 5000, 4)
    log.block("uniform", 30, 4)
    assert log.sample_room() == 10000  # (the oldest batch; the one being filled is smaller)
    log.pop()
    assert log.last == 10000 and log.sample_room() == 10000  # (a pipelined pipe delivers the popped batch's frames next)
    log.head(4, "uniform")
    log.pop()
    assert log.last == 30 and log.sample_room() == 30
