"""How the transposed Winograd form reads its block list (aivc_amd/csrc/wino_class_walk.h), without a GPU: the header is
compiled with the host compiler into tests/wino_class_walk_check.cpp's stand-alone program, which walks the list as the kernel's
persistent workgroups do and checks that every (pixel block, class, channel block) is computed exactly once for every list
length, channel-block count and grid it tries, and that the flagship launches deal every workgroup all classes evenly (read
the program's head for the grid and the bounds).  tests/test_gpu_winograd_class_walk.py has the bits."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_entry_once_and_classes_dealt_evenly(tmp_path):
    exe = str(tmp_path / 'wino_class_walk_check')
    cxx = os.environ.get('CXX', 'g++')
    subprocess.run([cxx, '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror', '-o', exe, os.path.join(HERE, 'wino_class_walk_check.cpp')],
                   check=True, timeout=120)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('ok: '), r.stdout
