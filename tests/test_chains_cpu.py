"""cppf_amd.chains without a device: the runners' chain cache (second sighting, least recently used, busy chains, a member that
leaves, the bounded sightings table), the split / full-first hysteresis and the chain-length policies, on fake pipelines and chains."""
import pytest

from cppf_amd import chains
from cppf_amd.chains import ChainCache


class Pipe:
    pass


class Chain:
    def __init__(self, pipes, tag):
        self.pipes, self.tag, self.released = list(pipes), tag, 0

    def release(self):
        self.released += 1


class Drain:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1


def make_cache(bound):
    drain = Drain()
    return ChainCache(bound, Chain, drain), drain


def key(pipes, tag=()):
    return tuple(id(p) for p in pipes) + tag


def test_second_sighting():
    cache, drain = make_cache(8)
    a = [Pipe(), Pipe()]
    assert cache.lookup(a) == (None, False) and len(cache) == 0 and not cache
    ch, capture = cache.lookup(a)
    assert ch.pipes == a and capture is True and len(cache) == 1
    assert cache.lookup(a) == (ch, True)
    b = [Pipe()]
    first, capture = cache.lookup(b, ("staged",), always=True)
    assert first.pipes == b and first.tag == ("staged",) and capture is False
    assert cache.lookup(b, ("staged",), always=True) == (first, True)
    # the staged tag is part of the key: the same pipelines without it are another combination
    assert cache.lookup(b) == (None, False)
    plain, capture = cache.lookup(b)
    assert plain is not first and capture is True and len(cache) == 3
    assert drain.calls == 0 and not any(c.released for c in cache.values())
    # always, on a combination that has been sighted before without it: captured at once
    c = [Pipe(), Pipe(), Pipe()]
    assert cache.lookup(c) == (None, False)
    assert cache.lookup(c, always=True)[1] is True


def twice(cache, pipes, **kw):
    cache.lookup(pipes, **kw)
    return cache.lookup(pipes, **kw)[0]


def test_least_recently_used_goes_first():
    cache, drain = make_cache(2)
    a, b, c, d = ([Pipe(), Pipe()] for _ in range(4))
    ca, cb = twice(cache, a), twice(cache, b)
    cc = twice(cache, c)
    assert (ca.released, cb.released, cc.released) == (1, 0, 0) and drain.calls == 1
    assert list(cache.values()) == [cb, cc]
    assert cache.lookup(b) == (cb, True)                  # a hit makes b the youngest
    cd = twice(cache, d)
    assert (cb.released, cc.released) == (0, 1) and drain.calls == 2
    assert list(cache.values()) == [cb, cd]


def test_busy_chains_are_not_evicted():
    cache, drain = make_cache(2)
    a, b, c, d = ([Pipe(), Pipe()] for _ in range(4))
    ca, cb = twice(cache, a), twice(cache, b)
    busy = set()
    assert cache.lookup(a, busy=busy) == (ca, True) and cache.lookup(b, busy=busy) == (cb, True)
    assert busy == {key(a), key(b)}
    assert cache.lookup(c, busy=busy) == (None, False)    # first sighting
    assert cache.lookup(c, busy=busy) == (None, False)    # second: every chain is busy, nothing is cached
    assert len(cache) == 2 and drain.calls == 0 and (ca.released, cb.released) == (0, 0) and busy == {key(a), key(b)}
    # one busy: the other goes, whichever is older -- here b is busy and a, the YOUNGER after the hit below, goes
    assert cache.lookup(a) == (ca, True)
    busy = {key(b)}
    cc, capture = cache.lookup(c, busy=busy)
    assert capture is True and (ca.released, cb.released) == (1, 0) and drain.calls == 1
    assert list(cache.values()) == [cb, cc] and busy == {key(b), key(c)}
    # and with the younger one busy the older goes
    busy = {key(c)}
    cd = twice(cache, d, busy=busy)
    assert (cb.released, cc.released, cd.released) == (1, 0, 0) and drain.calls == 2 and list(cache.values()) == [cc, cd]


def test_drop_member():
    cache, drain = make_cache(8)
    p, q, r, s = Pipe(), Pipe(), Pipe(), Pipe()
    cpq, cqr, crs = twice(cache, [p, q]), twice(cache, [q, r]), twice(cache, [r, s])
    cq = cache.lookup([q], ("staged",), always=True)[0]
    cache.drop_member(id(Pipe()))                         # no chain has it: no drain
    assert drain.calls == 0 and len(cache) == 4
    cache.drop_member(id(q))
    assert drain.calls == 1 and (cpq.released, cqr.released, cq.released, crs.released) == (1, 1, 1, 0)
    assert list(cache.values()) == [crs]
    cache.clear()
    assert crs.released == 1 and len(cache) == 0 and drain.calls == 2


def test_sightings_table_is_bounded_and_keeps_the_newcomer():
    """the table is cleared when it holds more than 4096 keys, BEFORE the new count is stored: the combination whose lookup finds it
    full keeps its sighting (stored after the clearing, the 4097th would lose its first sighting and never be captured)"""
    cache, _ = make_cache(4)
    pipes = [Pipe() for _ in range(4097)]
    for p in pipes:
        assert cache.lookup([p]) == (None, False)
    assert len(cache._sightings) == 4097                  # nothing lost so far
    ch, capture = cache.lookup([pipes[-1]])               # finds the table beyond its bound: cleared once, then counted
    assert ch is not None and capture is True
    assert cache._sightings == {key([pipes[-1]]): 2}
    assert cache.lookup([pipes[0]]) == (None, False)      # (forgotten with the rest: a first sighting again)


@pytest.mark.parametrize("start", [False, True])
def test_next_form(start):
    assert (chains.FULL_FIRST_ON, chains.FULL_FIRST_OFF) == (0.25, 0.10)
    want = {0.05: False, 0.10: start, 0.2: start, 0.25: start, 0.3: True}
    for share, form in want.items():
        assert chains.next_form(start, share) is form, share
        assert chains.next_form(start, share, split_ok=False) is True, share


def test_chain_lengths():
    assert [chains.resident_chain_len(n, 3) for n in (8, 16, 24, 1)] == [4, 8, 8, 1]
    assert [chains.host_chain_len(n, 3) for n in (8, 64)] == [1, 8]
    assert chains.frame_chain_len(6, 3, True) == 3 and chains.frame_chain_len(6, 3, False) == 2
    assert chains.frame_chain_len(3, 3, True) == 3 and chains.frame_chain_len(20, 3, True) == 7
    for n in range(0, 200):
        for lanes in (1, 2, 3, 4, 8):
            lens = (chains.resident_chain_len(n, lanes), chains.host_chain_len(n, lanes), chains.frame_chain_len(n, lanes, False),
                    chains.frame_chain_len(n, lanes, True))
            assert all(1 <= v <= 8 for v in lens), (n, lanes, lens)
