"""CPU suite of the chunk loop the per-item evaluations share (understanding_flow_robustness_amd/chunked_eval.py), with a subclass
that needs neither a device nor the library: what a chunk holds, when a new one starts, and what `read()` returns.  The evaluations'
own GPU tests (`test_items_of_another_size_start_a_new_chunk` in the *_gpu.py files) see the same rules through real launches."""
import numpy as np
import pytest
import torch

from understanding_flow_robustness_amd.chunked_eval import ChunkedEval, check_pair


class _Recorder(ChunkedEval):
    """Items are (key, value tensor [1,1]); a chunk's rows are (value, chunk number), and `chunks` keeps what each chunk held."""

    def __init__(self, chunk, two_tables=False):
        super().__init__(chunk)
        self.chunks, self.two_tables = [], two_tables

    def run_chunk(self, items):
        assert not torch.is_grad_enabled()
        self.chunks.append([(it[0], float(it[1])) for it in items])
        values = self.stack_f32([it[1] for it in items], torch.device("cpu"))
        rows = torch.cat((values, torch.full_like(values, len(self.chunks) - 1)), 1)
        return (rows, -rows) if self.two_tables else rows


def _feed(ev, keys):
    for i, key in enumerate(keys):
        ev.add(key, torch.tensor([[float(i)]], dtype=torch.float64))


def test_items_of_one_key_fill_chunks_of_chunk_items():
    ev = _Recorder(3)
    _feed(ev, ["a"] * 7)
    assert [len(c) for c in ev.chunks] == [3, 3] and len(ev.waiting) == 1       # a full chunk runs when the next item arrives
    (table,) = ev.read()
    assert [len(c) for c in ev.chunks] == [3, 3, 1] and ev.waiting == []
    assert table.dtype == np.float32 and table[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 6] and table[:, 1].tolist() == [0, 0, 0, 1, 1, 1, 2]


def test_a_key_change_starts_a_new_chunk_and_the_rows_keep_arrival_order():
    ev = _Recorder(4, two_tables=True)
    _feed(ev, ["a", "a", "b", "a", "a", "a", "a", "a"])
    rows, negated = ev.read()
    assert [[k for k, _ in c] for c in ev.chunks] == [["a", "a"], ["b"], ["a", "a", "a", "a"], ["a"]]
    assert [v for c in ev.chunks for _, v in c] == rows[:, 0].tolist() == list(range(8))
    assert rows[:, 1].tolist() == [0, 0, 1, 2, 2, 2, 2, 3] and np.array_equal(negated, -rows)


def test_read_flushes_only_once_and_an_empty_run_has_no_rows():
    ev = _Recorder(2)
    assert ev.read() == [] and ev.chunks == []
    ev.flush()
    assert ev.chunks == []
    _feed(ev, ["a"])
    assert len(ev.read()[0]) == 1 and len(ev.read()[0]) == 1 and len(ev.chunks) == 1


@pytest.mark.parametrize("chunk", [0, -1])
def test_a_chunk_below_one_is_refused(chunk):
    with pytest.raises(ValueError, match="^chunk must be positive$"):
        _Recorder(chunk)


def test_mark_records_nothing_without_an_event_list():
    ev = _Recorder(2)
    assert ev.events is None
    ev._mark("start")                       # with a list it would need a device: torch.cuda.Event
    _feed(ev, ["a", "a", "a"])
    ev.read()
    assert ev.events is None


def test_workspace_grows_and_is_kept():
    ev, cpu = _Recorder(2), torch.device("cpu")
    first = ev.workspace(8, cpu)
    assert first.dtype == torch.float64 and first.numel() == 8 and ev.workspace(5, cpu) is first
    assert ev.workspace(9, cpu).numel() == 9


def test_flow_shape_check_and_pair_check_keep_their_messages():
    flow = torch.zeros(4, 2, 8, 16)
    assert ChunkedEval.checked_flow(flow, 4, 6, 10) is flow and ChunkedEval.checked_flow(flow, 4, 8, 16, same_size=True) is flow
    for bad, kw in ((torch.zeros(3, 2, 8, 16), {}), (torch.zeros(4, 3, 8, 16), {}), (flow, dict(same_size=True))):
        with pytest.raises(RuntimeError, match=r"^the network returned a flow of shape \(\d, \d, 8, 16\) for 4 pairs of 6x10 frames$"):
            ChunkedEval.checked_flow(bad, 4, 6, 10, **kw)
    a = torch.zeros(1, 3, 4, 5)
    check_pair(a, a.clone(), "unused")
    for first, second in ((a[0], a[0]), (torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 4, 5)), (torch.zeros(1, 2, 4, 5), torch.zeros(1, 2, 4, 5)),
                          (a, torch.zeros(1, 3, 4, 6))):
        with pytest.raises(ValueError, match="^the caller's words$"):
            check_pair(first, second, "the caller's words")
