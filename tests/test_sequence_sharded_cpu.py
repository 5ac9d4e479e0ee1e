"""The rank ranges of a time-sharded window of the resident sequence (emba_amd.sharded.window_shard_ranges): batch_ranges on the WINDOW's batch grid,
shifted by the window's first event, with the (end - beg) % 100 tail on the last rank — what emba_group_set_events hands out on a host slice."""
from types import SimpleNamespace

import pytest

from emba_amd.driver import keeps_sequence
from emba_amd.sharded import BATCH, ShardedLEGM, ShardedModel, batch_ranges, window_shard_ranges

# (beg, end): a whole number of batches; a ragged tail; nb % world != 0 for worlds 2, 3 and 8 (nb = 301); fewer batches than ranks; an empty window
WINDOWS = [(0, 20_000), (137, 30_187), (1_300, 31_400), (500, 800), (700, 700), (42, 99)]


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_window_ranges_are_batch_ranges_shifted_with_the_tail_on_the_last_rank(world):
    seen_uneven = seen_tail = False
    for beg, end in WINDOWS:
        n = end - beg
        got = window_shard_ranges(beg, end, world)
        want = batch_ranges(n, world)
        assert len(got) == world
        for r, ((lo, hi), (wlo, whi)) in enumerate(zip(got, want)):
            assert lo == beg + wlo and (lo - beg) % BATCH == 0                       # on the window's grid, not the sequence's
            assert hi == (end if r == world - 1 else beg + whi)
        # contiguous, whole window
        assert got[0][0] == beg and got[-1][1] == end
        assert all(got[r][1] == got[r + 1][0] for r in range(world - 1))
        # the tail the library ignores sits on the last rank only
        assert got[-1][1] - (beg + want[-1][1]) == n % BATCH
        seen_uneven |= (n // BATCH) % world != 0
        seen_tail |= n % BATCH != 0
    assert seen_tail and (seen_uneven or world == 1)


def test_group_rule_is_the_same_rule():
    """emba_group_set_events[_seq]: nb / N batches each, the remainder on the first ranks."""
    for beg, end in WINDOWS:
        for world in (1, 2, 3, 8):
            nb, b = (end - beg) // BATCH, 0
            for r, (lo, hi) in enumerate(window_shard_ranges(beg, end, world)):
                cnt = nb // world + (1 if r < nb % world else 0)
                assert lo == beg + BATCH * b and hi == (end if r == world - 1 else beg + BATCH * (b + cnt))
                b += cnt


def test_run_sequence_keeps_host_slices_for_engines_without_a_resident_sequence():
    """driver.run_sequence decides by keeps_sequence(model): a ShardedModel over an engine without set_sequence (the CPU stand-in of tests/shard_engine.py)
    must go on getting host slices and the numpy blur, the same model over an engine that has one takes the resident path."""
    class Engine:
        def bind_exchange(self, count, pack):
            pass

    class DeviceEngine(Engine):
        def set_sequence(self, events, sampling_rate=1):
            return 0

    dist = SimpleNamespace(get_rank=lambda: 1, get_world_size=lambda: 3)
    legm = SimpleNamespace(H=4, W=8)
    host = ShardedModel(ShardedLEGM(Engine(), dist, None, None, 8), legm)
    assert hasattr(host, "set_sequence") and not host.has_resident_sequence and not keeps_sequence(host)
    assert keeps_sequence(ShardedModel(ShardedLEGM(DeviceEngine(), dist, None, None, 8), legm))
    assert keeps_sequence(SimpleNamespace(set_sequence=None)) and not keeps_sequence(SimpleNamespace(set_events=None))
    from shard_engine import OracleShardEngine
    assert not hasattr(OracleShardEngine, "set_sequence")
