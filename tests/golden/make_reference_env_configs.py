"""Writes tests/golden/reference_env_configs.json: every env config the reference ships
(config/env_configs/*.json, kept file for file under tests/golden/reference_env_configs/), loaded
through hftlob.config_io and re-serialised as our own dataclass dicts (asdict), so the GPU tests
can run each of them.
Usage: python tests/golden/make_reference_env_configs.py"""
import json
import os
import sys
from dataclasses import asdict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "jaxmarl-hft_amd"))
from hftlob.config_io import load_config_from_file  # noqa: E402

SRC = os.path.join(HERE, "reference_env_configs")
out = {f: asdict(load_config_from_file(os.path.join(SRC, f))) for f in sorted(os.listdir(SRC)) if f.endswith(".json")}
with open(os.path.join(HERE, "reference_env_configs.json"), "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
print(len(out), "configs")
