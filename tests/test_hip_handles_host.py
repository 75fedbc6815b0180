"""The two pieces every binding in graphlearning_amd._hip goes through, without a device: `call`, the checked library call that
names the function it ran, and `_Handle`, the one owner of a library object's lifetime (close, with, del, the closed-object refusal,
the objects abandoned at interpreter exit).  The library is a stand-in whose functions record their arguments and return a chosen
status."""
import ctypes
import gc
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from graphlearning_amd import _hip  # noqa: E402

HANDLE_CLASSES = ['DeviceGraph', 'Sweep', 'SweepGroups', 'Comm', 'DistSweep', 'Eig', 'Incres', 'Acq', 'KnnResult', 'BallResult']
CREATE = {'DeviceGraph': 'glx_graph_create', 'Sweep': 'glx_sweep_create', 'SweepGroups': 'glx_sweep_groups_create',
          'Comm': 'glx_dist_init_rank', 'DistSweep': 'glx_dist_sweep_create', 'Eig': 'glx_eig_create', 'Incres': 'glx_incres_create',
          'Acq': 'glx_acq_create', 'KnnResult': 'glx_knn_search', 'BallResult': 'glx_ball_search'}
ABANDONED = ['Comm', 'DistSweep']
LIFETIME_METHODS = ['close', '__del__', '__enter__', '__exit__', '_handle']


class FakeLib:
    """every glx_* function records (name, arguments) and returns `rc`; a create function (`handles` given) hands out the next handle"""

    def __init__(self, rc=0, err=b'', handles=None):
        self.rc, self.err, self.calls, self.handles = rc, err, [], handles

    def glx_last_error(self):
        return self.err

    def __getattr__(self, name):
        if not name.startswith('glx_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if self.rc == 0 and self.handles is not None and name in CREATE.values():
                args[-1]._obj.value = next(self.handles)         # (the byref of the out-parameter)
            return self.rc
        return fn


def install(monkeypatch, lib):
    monkeypatch.setattr(_hip, 'load', lambda required=True: lib)
    return lib


def with_handle(cls, value):
    obj = cls.__new__(cls)
    obj._h = ctypes.c_void_p(value)
    return obj


def test_the_handle_classes_are_the_ten_and_define_no_lifetime_of_their_own():
    found = [name for name, c in vars(_hip).items() if isinstance(c, type) and issubclass(c, _hip._Handle) and c is not _hip._Handle]
    assert sorted(found) == sorted(HANDLE_CLASSES)
    destroys = set()
    for name in HANDLE_CLASSES:
        cls = getattr(_hip, name)
        assert _hip._SIGNATURES[cls._destroy] == [ctypes.c_void_p], name
        destroys.add(cls._destroy)
        for method in LIFETIME_METHODS:
            assert method not in cls.__dict__, (name, method)
        assert _hip._SIGNATURES[CREATE[name]][-1] is ctypes.POINTER(ctypes.c_void_p), name      # what _open relies on
    assert len(destroys) == len(HANDLE_CLASSES)
    assert sorted(n for n in HANDLE_CLASSES if getattr(_hip, n)._abandon_at_exit) == sorted(ABANDONED)


@pytest.mark.parametrize('name', HANDLE_CLASSES)
def test_close_destroys_once_and_a_closed_object_is_refused(monkeypatch, name):
    cls = getattr(_hip, name)
    lib = install(monkeypatch, FakeLib())
    obj = with_handle(cls, 0x5000)
    assert obj._handle().value == 0x5000 and lib.calls == []
    obj.close()
    assert [(n, [a.value for a in args]) for n, args in lib.calls] == [(cls._destroy, [0x5000])]
    assert not obj._h.value
    obj.close()
    assert len(lib.calls) == 1
    with pytest.raises(_hip.GlxError, match='closed') as e:
        obj._handle()
    assert name in str(e.value) and str(e.value) == '%s: the object is closed' % name
    # a with block closes
    other = with_handle(cls, 0x6000)
    with other as inside:
        assert inside is other and other._handle().value == 0x6000
    assert not other._h.value and [n for n, _ in lib.calls] == [cls._destroy] * 2 and lib.calls[1][1][0].value == 0x6000
    with pytest.raises(_hip.GlxError, match='closed'):
        other._handle()


@pytest.mark.parametrize('name', HANDLE_CLASSES)
def test_close_without_the_library_and_del_without_a_handle(monkeypatch, capsys, name):
    cls = getattr(_hip, name)
    unraisable = []
    monkeypatch.setattr(sys, 'unraisablehook', unraisable.append)
    install(monkeypatch, None)                  # load(required=False) finds no library (interpreter shutdown, an unbuilt tree)
    obj = with_handle(cls, 0x7000)
    obj.close()
    assert not obj._h.value
    lib = install(monkeypatch, FakeLib())
    bare = cls.__new__(cls)                     # what __init__ leaves behind when it raises before the handle exists
    assert not hasattr(bare, '_h')
    bare.close()
    del bare
    gc.collect()
    assert lib.calls == [] and unraisable == [] and capsys.readouterr().err == ''


def test_open_appends_the_out_parameter_and_a_refused_create_leaves_the_object_closed(monkeypatch):
    lib = install(monkeypatch, FakeLib(handles=iter([0x100, 0x200])))
    obj = _hip.Eig.__new__(_hip.Eig)
    obj._open('glx_eig_create', 1, 2, 3)
    (name, args), = lib.calls
    assert name == 'glx_eig_create' and args[:3] == (1, 2, 3) and len(args) == 4 and args[3]._obj is obj._h
    assert obj._handle().value == 0x100
    obj.close()
    assert lib.calls[1][0] == 'glx_eig_destroy'
    bad = install(monkeypatch, FakeLib(rc=3, err=b'no memory'))
    failed = _hip.Acq.__new__(_hip.Acq)
    with pytest.raises(_hip.GlxError) as e:
        failed._open('glx_acq_create', 5)
    assert str(e.value) == 'glx_acq_create failed (3): no memory'
    assert not failed._h.value
    failed.close()
    assert [n for n, _ in bad.calls] == ['glx_acq_create']
    with pytest.raises(_hip.GlxError, match='Acq: the object is closed'):
        failed._handle()


def test_comm_and_dist_sweep_are_abandoned_at_exit_the_others_destroyed(monkeypatch):
    lib = install(monkeypatch, FakeLib(handles=iter(range(0x1000, 0x2000, 0x10))))
    objs = {}
    for name in HANDLE_CLASSES:
        cls = getattr(_hip, name)
        objs[name] = cls.__new__(cls)
        objs[name]._open(CREATE[name])          # the one place a handle comes from: nobody joins the table by hand
        assert objs[name]._handle().value
    lib.calls.clear()
    _hip._abandon_dist_objects()                # the atexit hook
    assert lib.calls == []
    for name in HANDLE_CLASSES:
        objs[name].close()
        assert not objs[name]._h.value
    assert sorted(n for n, _ in lib.calls) == sorted(getattr(_hip, n)._destroy for n in HANDLE_CLASSES if n not in ABANDONED)
    # closed in normal operation they are destroyed like every other object
    lib.calls.clear()
    for name in ABANDONED:
        cls = getattr(_hip, name)
        obj = cls.__new__(cls)
        obj._open(CREATE[name])
        obj.close()
    assert [n for n, _ in lib.calls if 'destroy' in n] == ['glx_dist_destroy', 'glx_dist_sweep_destroy']


def test_call_returns_none_or_raises_with_the_name_of_the_function_that_ran(monkeypatch):
    lib = install(monkeypatch, FakeLib())
    assert _hip.call('glx_eig_run', 1, 'x') is None
    assert lib.calls == [('glx_eig_run', (1, 'x'))]
    install(monkeypatch, FakeLib(rc=7, err=b'why'))
    with pytest.raises(_hip.GlxError) as e:
        _hip.call('glx_eig_run', None, 0, 1, None, None)
    assert str(e.value) == 'glx_eig_run failed (7): why'
    with pytest.raises(_hip.GlxError) as e:
        _hip.check(7, 'glx_eig_run')            # the primitive keeps its signature and its text
    assert str(e.value) == 'glx_eig_run failed (7): why'
    assert _hip.check(0, 'anything') is None


def test_the_three_misnamed_sites_report_the_function_that_ran(monkeypatch):
    monkeypatch.delenv('GLX_KNN_CLUSTERED', raising=False)
    lib = install(monkeypatch, FakeLib(rc=7, err=b'why'))
    with pytest.raises(_hip.GlxError, match=r'^glx_argmax_project_t failed \(7\): why$'):
        _hip.argmax_project(np.zeros((4, 2), dtype=np.float32))
    assert [n for n, _ in lib.calls] == ['glx_argmax_project_t']
    lib.calls.clear()
    with pytest.raises(_hip.GlxError, match=r'^glx_knn_bruteforce_range failed \(7\): why$'):
        _hip.knn_bruteforce(np.zeros((8, 2)), 2)
    assert [n for n, _ in lib.calls] == ['glx_knn_bruteforce_range']


def test_no_binding_names_its_function_twice():
    pkg = os.path.join(ROOT, 'graphlearning_amd')
    seen = 0
    for folder, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith('.py'):
                with open(os.path.join(folder, fn)) as f:
                    text = f.read()
                seen += 1
                for form in ('check(load()', 'check(lib.', '_hip.check(_hip.load()'):
                    assert form not in text, (fn, form)
    assert seen >= 2
