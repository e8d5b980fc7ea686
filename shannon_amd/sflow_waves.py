"""The sparse flow of the small partitions, in waves beside the graph stage: which thread starts a wave, when, and over which
partitions.  Knows threads and names only; the caller supplies the call that solves a wave (tests/test_sflow_waves.py drives the
rule with a fake one)."""
import threading


class WaveScheduler(object):
    """The thread that finishes a small partition's graph calls finished(name, record).  It takes every partition that is ready and
    in no wave yet, in `names` order, once there are `wave_min` of them, fewer than `waves_max` waves are running and at least
    `wave_min // 2` partitions are still to come -- or when this was the last partition, whatever is running.  A wave's rounds wait for
    the device, not for a core, so waves run beside the other threads' graphs; what counts is how little is left for the wave behind
    the LAST graph.  solve(names_in_order) -> texts runs on the calling thread; what it raises reaches that thread."""

    def __init__(self, names, wave_min, waves_max, solve):
        self.place = {nm: i for i, nm in enumerate(names)}
        self.wave_min, self.waves_max, self.solve = wave_min, waves_max, solve
        self.lock = threading.Lock()
        self.records, self.ready, self.done, self.waves_running = {}, [], 0, 0

    def finished(self, name, record):
        """-> [(name, text)] of the wave this thread ran, [] where it started none"""
        with self.lock:
            self.records[name] = record
            self.ready.append(name)
            self.done += 1
            left = len(self.place) - self.done
            if not (left == 0 or (len(self.ready) >= self.wave_min and self.waves_running < self.waves_max and left >= self.wave_min // 2)):
                return []
            wave, self.ready = sorted(self.ready, key=self.place.__getitem__), []
            self.waves_running += 1
        try:
            texts = self.solve(wave)
        finally:
            with self.lock:
                self.waves_running -= 1
        return list(zip(wave, texts))
