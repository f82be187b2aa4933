"""What the runners (batch.BatchPoseRunner, frames.FrameRunner) share around captured chains (inference.PoseChain): the bounded chain
cache, a chain's two forms, a group run with or without a chain, and how long a chain is.  Host logic only: tests/test_chains_cpu.py."""
from collections import OrderedDict

# Split or full-first (inference.PosePipeline): the form follows the survivor share of the last run, break-even ~0.15, with hysteresis.
FULL_FIRST_ON, FULL_FIRST_OFF = 0.25, 0.10


def next_form(full_first, share, split_ok=True):
    """-> full_first of the next run; split_ok=False (an encoder the fused second pass does not serve): full-first only"""
    if not split_ok or share > FULL_FIRST_ON:
        return True
    return False if share < FULL_FIRST_OFF else full_first


class ChainCache(OrderedDict):
    """The captured chains of a runner, least recently used first.  A chain is keyed by its members' id()s (+ `tag`) and made the
    SECOND time its combination comes up: a one-off combination runs its members' own graphs.
    make(pipes, tag) -> chain; drain(): called before any release() -- a victim may still have a replay in flight on its lane's stream."""

    def __init__(self, max_chains, make, drain):
        super().__init__()
        self.max_chains, self._make, self._drain, self._sightings = int(max_chains), make, drain, {}

    def lookup(self, pipes, tag=(), always=False, busy=None):
        """-> (chain or None, capture).  None: a combination seen for the first time, or a full cache whose every chain is in `busy`.
        always: a chain on the first sighting too, with capture=False (it then runs eagerly).  busy: a set of keys an eviction must not
        touch (the chains of the frame being enqueued); the returned chain's key is added to it.  busy=None: the oldest goes."""
        key, seen = tuple(id(p) for p in pipes) + tag, 2
        if key in self:
            self.move_to_end(key)
        else:
            seen = self._sightings.get(key, 0) + 1
            if len(self._sightings) > 4096:
                self._sightings.clear()
            self._sightings[key] = seen
            if seen < 2 and not always:
                return None, False
            while len(self) >= self.max_chains:
                victim = next((k for k in self if busy is None or k not in busy), None)
                if victim is None:
                    return None, False
                self._drop([victim])
            self[key] = self._make(pipes, tag)
        if busy is not None:
            busy.add(key)
        return self[key], seen >= 2

    def _drop(self, keys):
        if keys:
            self._drain()
        for k in keys:
            self.pop(k).release()

    def drop_member(self, pipe_id):
        """a pipeline leaves its runner: the chains it is a member of go with it"""
        self._drop([k for k in self if pipe_id in k])

    def clear(self):
        self._drop(list(self))


def refresh_images(encoders, point_encoders, categories, device):
    """The weight images of a batch's categories, looked at ONCE per batch on the caller's stream before the lanes fork from it: an
    update is re-packed in place now, ahead of every lane's replays, not by a lane on its own stream while its neighbours replay."""
    # (the groups then run with check_weights=None: a pipeline only compares the images' addresses, so a moved image re-captures)
    for cat in categories:
        if cat in encoders:
            encoders[cat]._packed_weights(device)
        if cat in point_encoders:
            point_encoders[cat]._packed_weights(device)


def run_group(chain, pipes, records, prestages=None):
    """Enqueue a group on the current stream: its chain, or without one every member's prestage (if any) and own graph.
    records: a device f64[21] per member that receives its record, or None (the caller collects them itself)."""
    if chain is not None:
        return chain.run_async(records, check_weights=None)
    for i, pipe in enumerate(pipes):
        if prestages is not None and prestages[i] is not None:
            prestages[i]()
        pipe.run_async(None if records is None else records[i], check_weights=None)


def adapt_group(chain, pipes, n_survs):
    """the split / full-first form of the group's next run from its members' survivor counts"""
    if chain is not None:
        return chain.adapt(n_survs)
    for pipe, n in zip(pipes, n_survs):
        pipe.adapt(n)


# Chain lengths, as measured.  Staged chains (objects resident on the device): chains of 1, 2, 4 or 8 members -- lists of equal length
# in those numbers keep each list on its own XCDs in the pair kernel (cppf_pair_mlp_batch_plan) -- the smallest such length that gives
# every lane at most one chain, capped at 8: 8 objects on 3 lanes run as 4 + 4 (0.145 ms per object; 3 + 3 + 2: 0.151, 2 + 2 + 2 + 2:
# 0.161), 16 as 8 + 8, 24 as 8 + 8 + 8 (profiles/r6_resident_probe.txt)
def resident_chain_len(n, n_lanes):
    return min(8, 1 << max(0, (-(-n // n_lanes) - 1).bit_length()))


# Host objects staged one by one: chains only when the batch keeps every lane two chains deep, because a small batch is bounded by the
# host staging it and a chain cannot start before its last member is staged (8 / 16 / 32 / 64 C2-size objects: no chains 0.189 / 0.163 /
# 0.164 / 0.158 ms per object, chains 0.193 / 0.164 / 0.161 / 0.140)
def host_chain_len(n, n_lanes):
    return max(1, min(8, n // (2 * n_lanes)))


# The instances of a frame.  batch_prestage (a chain's members share their frame stage): two chains of equal length on two lanes from
# four instances on, at most 8 members each (6 instances: 3 + 3 1.48 ms per frame, one chain 1.58, 2 + 2 + 2 1.50); without it chains
# of ceil(n / n_lanes), at most 8
def frame_chain_len(n, n_lanes, batch_prestage):
    if not batch_prestage:
        return max(1, min(8, -(-n // n_lanes)))
    n_chains = max(2 if n >= 4 and n_lanes > 1 else 1, -(-n // 8))
    return max(1, -(-n // n_chains))
