"""graphlearning_amd/csrc/size_class_pool.h, the size-class free list behind the device work-buffer pool and the page-locked block pool:
built on the host with ThreadSanitizer in front of counting stand-ins for the allocator (tests/size_class_pool_host.cpp)."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


@pytest.fixture(scope='module')
def driver():
    exe = os.path.join(tempfile.mkdtemp(), 'size_class_pool_host')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=thread', '-pthread', '-Wall', '-Werror',
                    '-I', os.path.join(ROOT, 'graphlearning_amd', 'csrc'), '-o', exe,
                    os.path.join(ROOT, 'tests', 'size_class_pool_host.cpp')], check=True)

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, TSAN_OPTIONS='halt_on_error=1'))
        assert r.returncode == 0 and 'ThreadSanitizer' not in r.stderr, (args, r.returncode, r.stderr[-4000:])
        return r.stdout
    return run


def device_class(b):
    """Power-of-two classes from 4 KiB to 64 MiB, then 16 MiB granules."""
    c = 4096
    while c < b:
        c <<= 1
    if c > 64 * MiB:
        c = -(-b // (16 * MiB)) * (16 * MiB)
    return c


def pinned_class(b):
    """Power-of-two classes from 4 KiB."""
    c = 4096
    while c < b:
        c <<= 1
    return c


def test_class_sizes_are_what_the_allocator_is_asked_for(driver):
    sizes = [0, 1, 4095, 4096, 4097, 4 * MiB - 1, 4 * MiB, 4 * MiB + 1, 64 * MiB - 1, 64 * MiB, 64 * MiB + 1, 100 * MiB, 256 * MiB + 1]
    lines = driver('classes', *sizes).split('\n')
    for b, line in zip(sizes, lines):
        got = [int(v) for v in line.split()]
        want_dev, want_pin = device_class(max(b, 1)), pinned_class(max(b, 1))
        assert got == [b, want_dev, want_dev, want_pin, want_pin], (b, got)


def test_idle_bytes_stay_within_the_caps(driver):
    driver('caps')


def test_disabled_pool_hands_every_block_back(driver):
    driver('disabled')


def test_out_of_memory_drains_and_retries_once(driver):
    driver('oom')


def test_concurrent_use_with_the_switch_toggled(driver):
    """8 threads x 10^5 allocations and frees while a ninth thread toggles the switch: clean under TSan, and after a final drain
    every block the allocator handed out went back to it."""
    out = driver('stress')
    assert 'allocations' in out
