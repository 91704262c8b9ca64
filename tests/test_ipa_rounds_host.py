"""The IPA rounds' field arithmetic (csrc/ipa_rounds.hpp: the rows of a round, the fold, the
verifier's scalars) without a GPU: tests/cpp/ipa_rounds_check.cpp, built with g++ and the address /
undefined-behaviour sanitizers and run directly. K = 0 .. 4 (N = 1 .. 16): every round's rows entry
by entry with and without the q terms, round 0's shortcut, every fold against a plain loop, the
coefficients against their closed form and points_coeffs, the verifier's scalars against the batched
verifier's closed forms (csrc/ipa_verify.hpp)."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_rounds_on_the_host(tmp_path):
    exe = tmp_path / "ipa_rounds_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "ipa_rounds_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    assert d["k_seen"] == 0b11111, d  # every K of 0 .. 4
    assert d["rows_bad"] == 0 and d["folds_bad"] == 0 and d["coeffs_bad"] == 0 and d["scalars_bad"] == 0, d
    # two runs per K: 4 N + 2 row entries per round (+ 2 N + 2 in round 0), 2 N coefficients per round
    assert d["rows"] == 2 * sum((4 * (1 << K) + 2) * K + (2 * (1 << K) + 2) * (K > 0) for K in range(5)), d
    assert d["coeffs"] == 2 * sum(2 * (1 << K) * K + (1 << K) for K in range(5)), d
    assert d["inner"] == 2 * 2 * 5 and d["inner_bad"] == 0, d  # inner against the plain dot, b dense and with zeros
    assert d["folds"] > 0 and d["scalars"] >= 2 * sum((1 << K) + 1 + 2 * K + 4 for K in range(5)), d
