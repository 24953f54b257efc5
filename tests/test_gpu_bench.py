"""bench.py's timed path on the GPU at a small size: the arrays it hands to
--dump-outputs are the last timed launch's, bit-exact against the oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("steps,per_call", [(5, 1), (6, 4), (8, 4)])
def test_timed_path_hands_back_its_last_launch(steps, per_call):
    """W warm-up + `steps` timed launches of one episode each, one or four
    per rollout call (a last call of 2 and of 4 launches): the outputs given
    to `after_timed` are episode W + steps of every game; a plain run makes
    no second pass."""
    import bench
    from rl_6_nimmt.vec_env import VecSechsNimmtEnv

    B, W = 300, 2  # ragged: not a multiple of a wave's games
    env = VecSechsNimmtEnv(B, bench.N_PLAYERS, seed=0, rng="numpy")
    env.reset()
    out = bench.make_out(env, B, True, per_call)
    got = {}
    wall, kern_ms, kt = bench.time_rollouts(env, out, steps, W, 1, per_call, kernel_pass=False,
                                            after_timed=lambda last: got.update(
                                                {k: v.cpu().numpy().copy() for k, v in last.items()}))
    assert wall > 0 and kern_ms is None and kt is None
    assert env.pipe_errors() == 0
    env.close()
    ref = O.VecOracle(B, bench.N_PLAYERS, rng_mode=O.RNG_NUMPY_MT, seed=0)
    ref.reset()
    for _ in range(W + steps):
        rr, rd, ra, ro = ref.rollout(bench.STEPS_PER_LAUNCH, want_obs=True)
    assert sorted(got) == ["actions", "done", "obs", "rewards"]
    assert np.array_equal(got["rewards"], rr)
    assert np.array_equal(got["done"], rd)
    assert np.array_equal(got["actions"], ra)
    assert np.array_equal(got["obs"][..., :47], ro)
