"""Host check of hmvec_amd/csrc/kernels/pb_map.hpp - the map from a linear block id of the batched mass integrals to
its (k tile, redshift): tests/cpp/pb_map_host.cpp includes the header the kernel includes and checks, for each of the
three orders, that the map is a bijection (all ntile, nz in 1..40 and the launch shapes (32,32), (64,4), (32,8), (1,1),
(1,65535), (33,7)), and the order's own properties: O1 never raises the tile with the id and deals every tile equally to
every class of id % 8 when nz is a multiple of 8; O2 opens with the highest and the lowest tile.  Built with g++ as a
stand-alone program, plainly and with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "pb_map_host.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_block_map_properties(tmp_path, flags):
    exe = tmp_path / "pb_map_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "pb_map ok" in r.stdout
