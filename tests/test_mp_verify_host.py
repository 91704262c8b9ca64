"""The multiproof many-verifier's shared text (csrc/mp_verify.hpp: the byte-stream SHA-256 feeder, the
fixed message layouts of t and of the inner IPA's challenges, the coefficient passes) without a GPU:
tests/cpp/mp_verify_check.cpp, built with g++ and the address / undefined-behaviour sanitizers
together with the library's host transcript (csrc/scheme_host.cpp) and run directly."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "verkle-kzg_amd", "csrc")


def test_mp_verify_text_on_the_host(tmp_path):
    exe = tmp_path / "mp_verify_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "mp_verify_check.cpp"), os.path.join(CSRC, "scheme_host.cpp"),
                           "-o", str(exe), "-lpthread"])
    out = subprocess.check_output([str(exe)], text=True, timeout=600)
    d = json.loads(out.splitlines()[-1])
    print(d)
    # r and t for every Q of 1 .. 130: every residue of the message length mod 64
    assert d["feeder"] == 2 * 130 and d["feeder_bad"] == 0, d
    assert d["residues"] == 64, d
    assert d["signs"] > 1000 and d["idents"] > 500, d  # of 8515 points: sign bits and identity flags were hashed
    assert d["inner"] == sum(1 + K for K in range(1, 9)) and d["inner_bad"] == 0, d
    assert d["coefs"] == 1 + 63 + 64 + 65 + 130 and d["coefs_bad"] == 0, d
    assert d["zero_denoms"] == 1, d
