"""The queue rules of sca_amd.scenes without a GPU: plan_slots (which entries the slots start with), next_episode (what a finished slot takes)
and a simulated stream over fixed episode lengths -- the recorded step counts 245, 284, 288 and 330, repeated -- held against running the
same queue in waves."""
import pytest

from sca_amd import scenes

LENGTHS = [245, 284, 288, 330]


def test_plan_slots_entry_i_in_slot_i():
    assert scenes.plan_slots([100] * 10, 4) == [0, 1, 2, 3]
    assert scenes.plan_slots([100] * 3, 8) == [0, 1, 2]                       # more slots than episodes: the queue's length
    assert scenes.plan_slots([], 4) == []


def test_plan_slots_reserves_a_slot_for_every_distinct_count():
    assert scenes.plan_slots([16] * 12 + [14, 14], 3) == [0, 1, 12]           # the first 14-agent episode takes the place of entry 2
    assert scenes.plan_slots([16, 14, 16, 16], 2) == [0, 1]
    assert scenes.plan_slots([8, 8, 8, 16, 100], 3) == [0, 3, 4]
    assert scenes.plan_slots([8, 8, 8, 16, 100], 4) == [0, 1, 3, 4]
    assert scenes.plan_slots([8, 16, 100], 3) == [0, 1, 2]
    with pytest.raises(ValueError):
        scenes.plan_slots([8, 16, 100], 2)
    with pytest.raises(ValueError):
        scenes.plan_slots([16, 14], 1)


def test_next_episode_order_and_exhaustion():
    assert scenes.next_episode(16, [16, 14, 16]) == 0                         # the first of its size
    assert scenes.next_episode(14, [16, 14, 16, 14]) == 1
    assert scenes.next_episode(100, [16, 14]) is None                         # none of its size: the slot stays done
    assert scenes.next_episode(16, []) is None
    pending, took = [14, 16, 16, 14], []
    while (k := scenes.next_episode(16, pending)) is not None:
        took.append(k)
        pending.pop(k)
    assert took == [1, 1] and pending == [14, 14]


def stream(sizes, lengths, slots):
    """the loop of run_episodes on episodes that last lengths[i] steps: (batch steps, [(slot, episode, first step)])"""
    holding = scenes.plan_slots(sizes, slots)
    pending = [i for i in range(len(sizes)) if i not in holding]
    left = [lengths[i] for i in holding]
    log = [(s, i, 0) for s, i in enumerate(holding)]
    steps = 0
    while any(h is not None for h in holding):
        steps += 1
        for s, i in enumerate(holding):
            if i is None:
                continue
            left[s] -= 1
            if left[s] == 0:
                k = scenes.next_episode(sizes[i], [sizes[j] for j in pending])
                holding[s] = None if k is None else pending.pop(k)
                if holding[s] is not None:
                    left[s] = lengths[holding[s]]
                    log.append((s, holding[s], steps))
    return steps, log


def waves(lengths, slots):
    """the same queue as waves of `slots` episodes, each wave as long as its slowest episode"""
    return sum(max(lengths[w:w + slots]) for w in range(0, len(lengths), slots))


@pytest.mark.parametrize('sizes,slots', [([16] * 16, 3), ([16] * 16, 4), ([16] * 16, 5), ([8, 16, 16, 16] * 4, 4), ([8, 16, 16, 16] * 4, 6)])
def test_simulated_stream(sizes, slots):
    lengths = LENGTHS * 4
    steps, log = stream(sizes, lengths, slots)
    assert sorted(i for _, i, _ in log) == list(range(16))                    # every episode runs exactly once
    slot_size = {}
    for s, i, _ in log:
        assert slot_size.setdefault(s, sizes[i]) == sizes[i], (s, i)         # no slot ever holds an episode of another size
    for s in set(s for s, _, _ in log):                                       # a slot's episodes follow each other without a gap
        mine = [(t, i) for q, i, t in log if q == s]
        for (t0, i0), (t1, _) in zip(mine, mine[1:]):
            assert t1 == t0 + lengths[i0]
    assert steps <= waves(lengths, slots), (steps, waves(lengths, slots))
    # by hand, three slots of one size: the waves last 288 + 330 + 330 + 330 + 288 + 330 steps; the stream's slots finish after
    # 245 + 330 + 245 + 288 + 284 = 1392, 284 + 245 + 288 + 284 + 245 + 330 = 1676 and 288 + 284 + 330 + 330 + 288 = 1520 steps (a slot that
    # finishes takes the first episode nobody has started)
    if slots == 3:
        assert waves(lengths, slots) == 1896 and steps == 1676
    if sizes[0] == 8 and slots == 4:                                          # one slot for the four 8-agent episodes: 4 x 245; the others 4 x 330 at most
        assert waves(lengths, slots) == 1320 and steps == 1320
