"""Trial sharding of the score / information calls (world_size 2, gloo, CPU), after the pattern of tests/test_dist_gloo.py.
The local evaluator is the dense CPU reference here (tests/fisher_ref.py) in the place of the HIP context; what is under test is
GPCSDModel's own sharding logic: the gather of the per-trial scores in trial order and the trial count of the expected information."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import torch.distributed as td
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    import fisher_ref as F
    from gpcsd_amd.dist import TrialSharding
    from gpcsd_amd.gpcsd1d import GPCSD1D
    from helpers import load_model_case
    c, g, geom, hp, lfp = load_model_case("1d_odd_17x37x5")
    hp = dict(hp, jitter=float(g["jitter"]))
    ref = F.scores_and_info(geom, hp, lfp)
    np.random.seed(0)
    m = GPCSD1D(lfp, c["x"], c["t"], a=c["a"], b=c["b"], ngl=c["ngl"])
    sh = TrialSharding()
    m.shard_trials(sh)
    sl = sh.local_slice(lfp.shape[2])

    class LocalEvaluator:                   # what _hip.Context offers the two methods, computed from this rank's trials alone
        def trial_scores(self, hp_, ntrials, ng):
            assert ntrials == sl.stop - sl.start
            return F.scores_and_info(geom, hp, lfp[:, :, sl])["scores"]

        def fisher(self, hp_, ng):
            return ref["info"].copy()

    m._fisher_args = lambda who: (LocalEvaluator(), None, None, ref["info"].shape[0])
    S = m.trial_scores()
    I = m.fisher_information(log_params=False)
    q.put((rank, (sl.start, sl.stop), float(np.max(np.abs(S - ref["scores"]) / (np.abs(ref["quad"]) + np.abs(ref["trace"])[None, :]))),
           bool(np.array_equal(S[sl], F.scores_and_info(geom, hp, lfp[:, :, sl])["scores"])),
           bool(np.array_equal(I, ref["info"] * float(lfp.shape[2]))), S.shape))
    td.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_scores_in_trial_order_and_total_trial_count_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(r[1] for r in res) == [(0, 3), (3, 5)]
    for rank, block, err, own_bits, info_ok, shape in res:
        assert shape == (5, 5)
        assert err < 1e-9          # every rank holds all five trials' scores at their own rows (dense solves of 3 or 2 trials against 5)
        assert own_bits            # ... and its own block bit for bit: the gather adds zeros
        assert info_ok             # the expected information counts all trials, not the local block
