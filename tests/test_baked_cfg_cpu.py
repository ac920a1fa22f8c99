"""The baked-config table (jaxmarl-hft_amd/csrc/baked_cfgs.inc) and the library's match of a caller's
config against it (hftlob_env_baked_id), host-only.

The committed table is what tools/gen_baked_cfg.py writes today from hftlob/configs through the
package's packer; every packed builtin config matches its own entry (whatever the day's n_windows
and n_data_rows are); one changed word of the lob block, of the world words or of types[1] matches
nothing; the switch hftlob_set_baked turns the match off."""
import ctypes as C
import importlib.util
import os

import pytest

from hftlob import _lib
from hftlob.config_io import builtin_config
from hftlob.layout import pack_env_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen():
    spec = importlib.util.spec_from_file_location("gen_baked_cfg", os.path.join(ROOT, "tools", "gen_baked_cfg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _packed(name, n_windows=4, n_data_rows=1000):
    return pack_env_cfg(builtin_config(name), n_windows, n_data_rows, True)[0]


def _id(c):
    return int(_lib.lib().hftlob_env_baked_id(C.byref(c)))


def test_committed_table_is_the_generators_output():
    g = _gen()
    with open(g.OUT) as f:
        assert f.read() == g.render(), "baked_cfgs.inc is stale: run tools/gen_baked_cfg.py"
    names = g.builtin_names()
    assert sorted(n + ".json" for n in names) == sorted(os.listdir(os.path.join(ROOT, "jaxmarl-hft_amd", "hftlob",
                                                                                "configs")))
    assert names[:2] == ["2_player_fq_fqc", "3_player_fq_fqc_dir"], "the ids the library has kernels for"


def test_generator_writes_the_packers_bits():
    """floats as hex-float literals of the packed float32, the pre-rounded fields the packer's"""
    g = _gen()
    c = _packed("2_player_fq_fqc")
    text = g.render()
    for f in ("rebate_factor", "one_minus_eta", "reward_scaling_quo"):
        v = getattr(c.types[0], f)
        assert float.fromhex(float(v).hex()) == v
        assert f"/* {f} */ {float(v).hex()}f" in text
    assert f"/* tick_magic */ {g.tick_magic(c.tick_size)}u" in text
    from test_abi import tick_magic
    assert g.tick_magic(100) == tick_magic(100) and g.tick_magic(25) == tick_magic(25) and g.tick_magic(1) == tick_magic(1)


@pytest.mark.parametrize("i,name", list(enumerate(_gen().builtin_names())))
def test_baked_id_of_builtin_configs(i, name):
    assert _id(_packed(name)) == i
    assert _id(_packed(name, n_windows=1, n_data_rows=123_456)) == i, "the day's words are not compared"
    c = _packed(name)
    c.tick_magic = 12345                                            # (the library sets its own)
    assert _id(c) == i


@pytest.mark.parametrize("group", ["lob", "world", "types1"])
def test_baked_id_minus_one_after_one_changed_word(group):
    for name in ("2_player_fq_fqc", "3_player_fq_fqc_dir"):
        c = _packed(name)
        if group == "lob":
            c.lob.book_depth += 1
        elif group == "world":
            c.order_id_counter_start -= 1
        else:
            c.types[1].task_size += 1
        assert _lib.lib().hftlob_env_launch_info(C.byref(c), C.byref(_lib.LaunchInfo())) == 0, "still a valid config"
        assert _id(c) == -1


def test_switch():
    c = _packed("2_player_fq_fqc")
    assert _lib.set_baked(False) is True, "the default is on"
    try:
        assert _id(c) == -1
    finally:
        assert _lib.set_baked(True) is False
    assert _id(c) == 0
