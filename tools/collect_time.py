"""What a step of the three device loops costs by the wall clock (Python that issues torch operations and library calls around the step kernel), through the
public API only, so that the same file runs on any commit: 4096 ReachHuman envs (SSM shield, horizon 100), fixed action tensors as the policy (no learner cost),
  * collect_rollout at n_steps 64 (zeros as values and log-probabilities);
  * collect_steps(., 100) into a replay buffer;
  * collect_steps(., 100) into a hindsight buffer on the goal env.
After a warm-up block, seven blocks each, by the wall clock around a block that ends in torch.cuda.synchronize(); ms per env step.
python tools/collect_time.py [--label NAME] [--out PATH] [--n-envs N]        one run, of the package in the working directory
python tools/collect_time.py --merge BASE NEW BASE NEW --out PATH          four runs (one process each, in that order) into one file with the verdict: for each
loop, the new commit's larger median may exceed the slower of the base's two medians by no more than the base's block-to-block spread (max - min over the
blocks of a run, the larger of its two runs): the noise floor of a wall-clock figure on a shared machine."""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, '.')


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def write(path, out):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def merge(paths, out_path):
    runs = [json.load(open(p)) for p in paths]
    base, new, verdict = runs[0::2], runs[1::2], {}
    for loop in runs[0]["ms_per_step"]:
        slower = max(r["median_ms"][loop] for r in base)
        spread = max(r["spread_ms"][loop] for r in base)
        worst = max(r["median_ms"][loop] for r in new)
        verdict[loop] = dict(base_slower_median_ms=slower, base_spread_ms=spread, new_median_ms=[r["median_ms"][loop] for r in new], excess_ms=worst - slower,
                             within_noise=bool(worst - slower <= spread))
        print("%-16s base %.4f ms (spread %.4f), new %s: %s" % (loop, slower, spread, " ".join("%.4f" % r["median_ms"][loop] for r in new),
                                                                 "within the noise" if verdict[loop]["within_noise"] else "SLOWER"))
    write(out_path, dict(order=[r["label"] for r in runs], verdict=verdict, runs=runs))
    return all(v["within_noise"] for v in verdict.values())


if "--merge" in sys.argv:
    i = sys.argv.index("--merge")
    sys.exit(0 if merge(sys.argv[i + 1:i + 5], arg("--out", "profiles/collect_time.json")) else 1)

import torch   # noqa: E402
import human_robot_gym_amd as hrg   # noqa: E402

n, blocks = arg("--n-envs", 4096), 7
kw = dict(env_kwargs=dict(shield_type="SSM", horizon=100, seed=1234))


def clock(fn, steps):
    """ms per step of one warm-up block (dropped) and `blocks` timed blocks of `steps` steps."""
    ms = []
    for _ in range(blocks + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    return ms[1:]


def fixed_actions(env):
    A = env.action_space.shape[0]
    return torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (n, A)).astype(np.float32)).cuda()


ms = {}
env = hrg.HipVecEnv(n, **kw)
env.attach_rollout(64)
acts, zeros = fixed_actions(env), torch.zeros(n, device="cuda")
ms["collect_rollout"] = clock(lambda: env.collect_rollout(lambda obs: (acts, zeros, zeros), lambda obs: zeros), 64)
env.close()
env = hrg.HipVecEnv(n, **kw)
env.attach_replay(128 * n)
acts = fixed_actions(env)
ms["collect_steps_replay"] = clock(lambda: env.collect_steps(lambda obs: acts, 100), 100)
env.close()
env = hrg.HipVecEnv(n, goal_env=True, **kw)
env.attach_her(128)
acts = fixed_actions(env)
ms["collect_steps_her"] = clock(lambda: env.collect_steps(lambda obs: acts, 100), 100)
env.close()
out = dict(label=arg("--label", "run"), n_envs=n, blocks=blocks, ms_per_step=ms, median_ms={k: float(np.median(v)) for k, v in ms.items()},
           spread_ms={k: float(np.max(v) - np.min(v)) for k, v in ms.items()})
for k, v in ms.items():
    print("%-20s ms per %d-env step: %s  median %.4f  spread %.4f" % (k, n, " ".join("%.4f" % x for x in v), out["median_ms"][k], out["spread_ms"][k]))
write(arg("--out", "profiles/collect_time_run.json"), out)
