"""_lib.load keeps one bound handle per library file, so several builds of the library live side by side in
one process (Sim(lib=...)); no GPU needed.  A byte copy of libmmx.so under another name stands for a second
build: the same exported names, its own statics.  A stub with two exports stands for a library of an older
revision."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

STUB = """
extern "C" const char* mmx_last_error(const void*) { return "stub"; }
extern "C" unsigned mmx_episode_seed(unsigned long long root, int index) { return (unsigned)root + index; }
"""


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    out = tmp_path_factory.mktemp("stub") / "libstub.so"
    src = out.with_suffix(".cpp")
    src.write_text(STUB)
    subprocess.check_call(["g++", "-shared", "-fPIC", "-o", str(out), str(src)])
    return out


def test_a_copy_is_a_second_handle(tmp_path):
    from mujoco_manip_amd import _build, _lib

    default = _lib.load()
    assert _lib.load(None) is default and _lib.load(build_if_missing=False) is default
    copy = tmp_path / "libmmx_copy.so"
    shutil.copy(_build.LIB, copy)  # (a link would be the same object to the loader)
    other = _lib.load(str(copy))
    assert other is not default and other._handle != default._handle
    assert _lib.load(str(copy)) is other  # cached per file, whatever the spelling of its path
    assert _lib.load(str(tmp_path / "." / "libmmx_copy.so")) is other
    assert _lib.load() is default and _lib.load(None) is default
    assert _lib.load(default._name) is default
    for L in (default, other):
        for name in _lib.EXPORTED:
            restype, argtypes = _lib._PROTOS[name]
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    want = int(np.random.SeedSequence(42).spawn(4)[3].generate_state(1)[0])
    assert default.mmx_episode_seed(42, 3) == other.mmx_episode_seed(42, 3) == want
    for L in (default, other):  # each answers for itself, with no device
        cfg = _lib.MMXConfig()
        L.mmx_config_default(C.byref(cfg))
        cfg.num_envs = 0
        ptr = C.c_void_p()
        assert L.mmx_create(C.byref(cfg), C.byref(ptr)) == -1 and not ptr.value  # MMX_EINVAL


def test_a_missing_path_raises(tmp_path):
    from mujoco_manip_amd import _lib

    with pytest.raises(RuntimeError, match=r"libmmx_none\.so.*__graft_entry__\.build\(\)"):
        _lib.load(str(tmp_path / "libmmx_none.so"))
    with pytest.raises(RuntimeError):  # build_if_missing is about the default only
        _lib.load(str(tmp_path / "libmmx_none.so"), build_if_missing=True)


def test_a_library_named_by_path_is_bound_with_the_names_it_has(stub):
    from mujoco_manip_amd import _lib

    L = _lib.load(str(stub))
    assert L.mmx_last_error(None) == b"stub"  # bound with _PROTOS' types: bytes, not an int
    assert L.mmx_episode_seed(40, 2) == 42
    with pytest.raises(AttributeError):
        L.mmx_create


def test_the_in_tree_library_must_export_every_name(stub, tmp_path, monkeypatch):
    from mujoco_manip_amd import _build, _lib

    product = tmp_path / "libmmx.so"
    shutil.copy(stub, product)
    monkeypatch.setattr(_build, "LIB", str(product))
    with pytest.raises(AttributeError):
        _lib.load(str(product))
