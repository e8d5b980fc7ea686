"""The sparse-flow wave rule (shannon_amd/sflow_waves.py) on its own, with a fake solve: which call of finished() starts a wave, over
which partitions, and how many waves are open at once.  No device, no native code."""
import queue
import random
import threading

import pytest

from shannon_amd.sflow_waves import WaveScheduler

WAIT = 10.0         # seconds an event may take before a test fails; nothing here waits that long when the code is right


def _names(n):
    return ["p%03d" % i for i in range(n)]


@pytest.mark.parametrize("n_small, wave_min, waves_max, sizes", [
    (40, 16, 4, [16, 16, 8]),
    (36, 16, 4, [16, 20]),          # after the 32nd only 4 are left, below wave_min // 2: they wait for the last
    (10, 16, 4, [10]),
    (1, 16, 4, [1]),
])
def test_waves_from_one_thread(n_small, wave_min, waves_max, sizes):
    # solve returns at once: no wave is running at any decision, the waves follow from the rule alone
    names, waves = _names(n_small), []

    def solve(wave):
        waves.append(list(wave))
        return ["text of " + nm for nm in wave]
    sched = WaveScheduler(names, wave_min, waves_max, solve)
    order = list(names)
    random.Random(7).shuffle(order)
    got = {}
    for nm in order:
        pairs = sched.finished(nm, {"record of": nm})
        assert sched.waves_running == 0
        for name, text in pairs:
            assert name not in got
            got[name] = text
    assert [len(w) for w in waves] == sizes
    assert sorted(nm for w in waves for nm in w) == names                   # each name in exactly one wave
    for w in waves:
        assert w == sorted(w, key=names.index)                              # in `names` order, whatever order they finished in
    assert got == {nm: "text of " + nm for nm in names}
    assert all(sched.records[nm] == {"record of": nm} for nm in names)


def test_waves_in_flight_are_capped_but_the_last_partition_always_starts_one():
    names, n, wave_min, waves_max = _names(80), 80, 16, 2
    release, events, lock = threading.Event(), queue.Queue(), threading.Lock()
    open_now, open_max, texts, threads = [0], [0], {}, []

    def solve(wave):
        with lock:
            open_now[0] += 1
            open_max[0] = max(open_max[0], open_now[0])
            events.put(("wave", list(wave), open_now[0]))
        assert release.wait(WAIT), "the test never released the waves"
        with lock:
            open_now[0] -= 1
        return ["text of " + nm for nm in wave]
    sched = WaveScheduler(names, wave_min, waves_max, solve)

    def finish(nm):
        pairs = sched.finished(nm, None)
        with lock:
            texts.update(pairs)
        events.put(("returned", nm, pairs))
    started = {}
    for i, nm in enumerate(names):
        # one partition at a time: its thread either comes back with no wave or is held inside solve
        t = threading.Thread(target=finish, args=(nm,), daemon=True)
        t.start()
        threads.append(t)
        ev = events.get(timeout=WAIT)
        if ev[0] == "wave":
            started[i + 1] = ev
        else:
            assert ev[1] == nm and ev[2] == []
    # waves behind the 16th and the 32nd partition; with two open none behind the 48th or the 64th though partitions remain; the
    # partition that finishes last starts its wave whatever is running
    assert sorted(started) == [16, 32, 80]
    assert [started[k][2] for k in (16, 32, 80)] == [1, 2, 3] and sched.waves_running == 3
    assert started[16][1] == names[:16] and started[32][1] == names[16:32] and started[80][1] == names[32:]
    release.set()
    for t in threads:
        t.join(WAIT)
        assert not t.is_alive()
    assert open_max[0] == waves_max + 1 and sched.waves_running == 0
    assert texts == {nm: "text of " + nm for nm in names}


def test_a_failing_solve_reaches_its_caller_and_frees_its_place():
    names, calls = _names(40), []

    def solve(wave):
        calls.append(list(wave))
        if len(calls) == 1:
            raise RuntimeError("no room for the LP batch")
        return ["text of " + nm for nm in wave]
    sched = WaveScheduler(names, 16, 1, solve)
    for nm in names[:15]:
        assert sched.finished(nm, None) == []
    with pytest.raises(RuntimeError, match="no room for the LP batch"):
        sched.finished(names[15], None)
    assert sched.waves_running == 0
    # ... so with waves_max = 1 the next wave still starts
    got = [pair for nm in names[16:] for pair in sched.finished(nm, None)]
    assert [len(w) for w in calls] == [16, 16, 8] and [nm for nm, _ in got] == names[16:]
