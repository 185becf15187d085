"""TEST INFRASTRUCTURE: what tests/mock_gpu/Makefile builds, made once per Python process into one temporary directory.

host_lib() is the product's host sources over the CPU stand-ins of the device ABI, gpu_lib() the stand-ins themselves
(the library host_lib() is linked against, so its test hooks count what the host side called).  Both are loaded once:
their counters are process-wide, and a test that reads one takes a difference.  program() and rules() build one named
target of the Makefile and give its path.  A module that routes la_api to host_lib() still brackets its tests with
la_api.use_library(lib) / la_api.use_library(None) itself."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

MOCK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mock_gpu")
JOBS = "-j%d" % min(8, os.cpu_count() or 1)


@functools.lru_cache(maxsize=None)
def out_dir():
    d = tempfile.mkdtemp(prefix="la_mock_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def _built(target):
    path = os.path.join(out_dir(), target)
    subprocess.check_call(["make", "-s", JOBS, "-C", MOCK_DIR, "OUT=" + out_dir(), path])
    return path


@functools.lru_cache(maxsize=None)
def host_lib():
    """libla_host_mock.so, loaded (it finds libla_gpu_mock.so beside itself)"""
    return C.CDLL(_built("libla_host_mock.so"))


@functools.lru_cache(maxsize=None)
def gpu_lib():
    """libla_gpu_mock.so, loaded: every stand-in and every test hook"""
    return C.CDLL(_built("libla_gpu_mock.so"))


def program(name):
    """the path of a program of the Makefile: la_read_asan, {bzip2,xz,lzip,zip}_write_asan, deflate_find_asan,
    lzo_rules_bench"""
    return _built(name)


def rules(name):
    """the path of a rules object of the Makefile, which compiles a kernel's rules header and no host code:
    libxz_rules.so, liblzip_rules.so, libdeflate_find_rules.so"""
    return _built(name)
