"""sharding.placement: device index, `shared` and the default backend as a pure function of the launcher's environment and the
number of GPUs on the node -- no process group, no GPU.  A multi-node launch that names no ranks per node used to take gloo with
host staging on every rank without a word; the ranks per node now come from LOCAL_WORLD_SIZE, OMPI_COMM_WORLD_LOCAL_SIZE or
SLURM_NTASKS_PER_NODE, and the WORLD_SIZE guess warns when it is what makes the ranks share devices."""
import warnings

import pytest

from cppf_amd import sharding

LOCAL_SIZE_VARS = ("LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "SLURM_NTASKS_PER_NODE")


def place(env, n_dev):
    """-> (local, shared, backend, [warning messages])"""
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        out = sharding.placement(env, n_dev)
    return out + ([str(w.message) for w in seen],)


def test_sixteen_ranks_on_eight_devices_with_nothing_set_warn_and_take_gloo():
    for local_rank in (0, 5, 7):
        local, shared, backend, seen = place(dict(WORLD_SIZE="16", RANK=str(8 + local_rank), LOCAL_RANK=str(local_rank)), 8)
        assert (local, shared, backend) == (local_rank, True, "gloo")                    # as before: LOCAL_RANK mod 8, gloo
        assert len(seen) == 1
        assert "LOCAL_WORLD_SIZE" in seen[0] and "gloo" in seen[0] and "host staging" in seen[0]


@pytest.mark.parametrize("name", LOCAL_SIZE_VARS)
def test_sixteen_ranks_on_eight_devices_with_the_ranks_per_node_named_take_rccl(name):
    for rank in range(16):
        env = {"WORLD_SIZE": "16", "RANK": str(rank), "LOCAL_RANK": str(rank % 8), name: "8"}
        assert place(env, 8) == (rank % 8, False, "nccl", [])


def test_the_first_variable_that_is_set_wins():
    env = dict(WORLD_SIZE="16", LOCAL_RANK="3", LOCAL_WORLD_SIZE="8", OMPI_COMM_WORLD_LOCAL_SIZE="16", SLURM_NTASKS_PER_NODE="16")
    assert place(env, 8) == (3, False, "nccl", [])
    env = dict(WORLD_SIZE="16", LOCAL_RANK="3", LOCAL_WORLD_SIZE="", OMPI_COMM_WORLD_LOCAL_SIZE="8", SLURM_NTASKS_PER_NODE="16")
    assert place(env, 8) == (3, False, "nccl", [])
    env = dict(WORLD_SIZE="16", LOCAL_RANK="11", SLURM_NTASKS_PER_NODE="16")            # 16 ranks really on one 8-GPU node
    assert place(env, 8) == (3, True, "gloo", [])


def test_two_ranks_on_one_device_share_it_over_gloo():
    for local_rank in (0, 1):
        env = dict(WORLD_SIZE="2", RANK=str(local_rank), LOCAL_RANK=str(local_rank), LOCAL_WORLD_SIZE="2")
        assert place(env, 1) == (0, True, "gloo", [])
    local, shared, backend, seen = place(dict(WORLD_SIZE="2", RANK="1", LOCAL_RANK="1"), 1)      # the guess is right here, but it is a guess
    assert (local, shared, backend) == (0, True, "gloo") and len(seen) == 1


def test_one_rank_and_full_nodes_are_unchanged():
    assert place({}, 1) == (0, False, "nccl", [])
    assert place({}, 8) == (0, False, "nccl", [])
    assert place(dict(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), 1) == (0, False, "nccl", [])
    assert place({}, 0) == (0, False, "gloo", [])                                         # no GPU: gloo, nothing shared
    assert place(dict(WORLD_SIZE="2", LOCAL_RANK="1"), 0) == (1, False, "gloo", [])
    for local_rank in range(8):                                                           # one full node, no LOCAL_WORLD_SIZE
        assert place(dict(WORLD_SIZE="8", LOCAL_RANK=str(local_rank)), 8) == (local_rank, False, "nccl", [])


def test_init_distributed_uses_the_placement(monkeypatch):
    """a single rank creates no group: init_distributed returns what placement() decides for the process's own environment"""
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CPPF_FORCE_DIST") + LOCAL_SIZE_VARS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LOCAL_RANK", "0")
    assert sharding.init_distributed(force=False) == (0, 1, 0)
