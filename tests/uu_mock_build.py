"""TEST INFRASTRUCTURE: what tests/mock_gpu/uu.mk builds -- the libraries of tests/mock_build.py with the uu read filter
and the stand-in of la_gpu_uu_decode added -- made once per Python process into a temporary directory of its own, so
that the libraries mock_build.py loads stay what they were.  Same interface: host_lib(), gpu_lib(), program(name)."""
import atexit
import ctypes as C
import functools
import shutil
import subprocess
import tempfile

from mock_build import JOBS, MOCK_DIR


@functools.lru_cache(maxsize=None)
def out_dir():
    d = tempfile.mkdtemp(prefix="la_mock_uu_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def _built(target):
    path = out_dir() + "/" + target
    subprocess.check_call(["make", "-s", JOBS, "-C", MOCK_DIR, "-f", "uu.mk", "OUT=" + out_dir(), path])
    return path


@functools.lru_cache(maxsize=None)
def host_lib():
    """libla_host_mock_uu.so: the host sources with la_filter_uu.c, loaded (it finds libla_gpu_mock_uu.so beside itself)"""
    return C.CDLL(_built("libla_host_mock_uu.so"))


@functools.lru_cache(maxsize=None)
def gpu_lib():
    """libla_gpu_mock_uu.so: every stand-in and the uu one, loaded"""
    return C.CDLL(_built("libla_gpu_mock_uu.so"))


def program(name):
    """the path of a program: la_read_asan (with the uu filter), uu_rules_bench"""
    return _built(name)
