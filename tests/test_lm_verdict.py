"""The LM decision code the kernels share (`vors::lm_verdict`, csrc/lie.h: eval's accept test + stop_criterion + the lm_coef update,
lm_optimizer.rs:140-192) against the oracle's own `LMOptimizerState::eval` and `stop_criterion`, on the CPU: lie.h is host + device
code, so the very function every kernel form calls is compiled for the host by oracle/lm_verdict_check.cpp and walked over a grid —
nb_iter in {0, 1, 20, 21, 22}; candidate energy below / equal / above the kept one, apart by exactly 1.0f and by its two neighbours,
NaN on either side, infinite kept energies; lm_coef in {0.1, 1e-8, 1e8, a denormal, one that overflows}. Required: the same one of the
four verdicts and the same lm_coef bits in every case."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")


def test_lm_verdict_equals_oracle_eval_and_stop_criterion_on_grid():
    subprocess.check_call(["make", "-C", ORACLE, "-s", "lm_verdict_check"])  # (no-op when up to date with lie.h and the oracle header)
    out = subprocess.run([os.path.join(ORACLE, "lm_verdict_check")], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"lm_verdict vs oracle: (\d+) cases, (\d+) mismatches", out.stdout)
    assert m and int(m.group(2)) == 0
    # the whole grid ran: 3 finite candidate energies x 13 kept energies + NaN x 4, times 5 iteration counts x 5 coefficients
    assert int(m.group(1)) == (3 * 13 + 4) * 5 * 5
    for verdict in ("rejected, go on", "rejected, stop", "accepted, go on", "accepted, stop"):
        n = re.search(re.escape(verdict) + r"\s+(\d+) cases", out.stdout)
        assert n and int(n.group(1)) > 0, f"the grid never reached '{verdict}'"
