"""How the persistent Winograd workgroups claim the entries of the block list at run time (aivc_amd/csrc/wino_dynamic_walk.h),
without a GPU: the header is compiled with the host compiler into tests/wino_dynamic_walk_check.cpp's stand-alone program, which
runs the workgroups' protocol on the counters as a simulation, one fetch-and-add per step, in seeded random interleavings --
all workgroups resident, fewer resident than the grid (down to one at a time), a third of the grid started only after every
other workgroup has left -- and checks that every entry is claimed exactly once and none outside the list, in all three
forms' readings of an entry, that every workgroup terminates, and that the counters are zero after the last exit (read the
program's head for the lists and grids).  tests/test_gpu_winograd_dynamic_walk.py has the bits."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_entry_claimed_once_and_counters_left_zero(tmp_path):
    exe = str(tmp_path / 'wino_dynamic_walk_check')
    cxx = os.environ.get('CXX', 'g++')
    subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(HERE, 'wino_dynamic_walk_check.cpp')],
                   check=True, timeout=120)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith('ok: '), r.stdout
