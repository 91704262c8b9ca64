"""Montgomery's trick over block products on the host (csrc/batch_inv.hpp BlockInverses: the host
step of normalize.hip's split normalisations and of poly.hip's batch_inverse), built with g++ and
the address / undefined-behaviour sanitizers and run directly: BN254 Fq, BLS12-381 Fq, Bandersnatch's
base field and BN254 Fr, nblk = 1, 2, 3 and 127, in one take, in uneven pieces with empty takes and
one block at a time, products equal to one included (tests/cpp/batch_inv_check.cpp)."""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_block_inverses_match_single_inversions(tmp_path):
    exe = tmp_path / "batch_inv_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(HERE, "cpp", "batch_inv_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True, timeout=120)
    res = {d["field"]: d for d in map(json.loads, out.splitlines())}
    assert set(res) == {"bn254_fq", "bls12_381_fq", "bandersnatch_fq", "bn254_fr"}
    for name, d in res.items():
        assert d["checks"] == 3 * 3 * (1 + 2 + 3 + 127), d
        assert d["mismatches"] == 0, d
