"""The kernel families the fp16 DenseNet-121 encoder really launches (DenseNet121Features.profile()) against
tests/golden/encoder_routes.json, for the table's two-frame entries at 224 and 232: created under the entry's TN_* environment, the
encoder launches what the fixture - and through tests/test_cpu_encoder_routes.py the device-free plan, tn_dbg_encoder_plan - says."""
import json
import os

import pytest
import torch

from tennis_amd import weights as W
from tennis_amd.engine import DenseNet121Features
from test_cpu_encoder_routes import FIXTURE, SWITCHES, entry_id

pytestmark = pytest.mark.gpu

with open(FIXTURE) as _f:
    ENTRIES = [e for e in json.load(_f) if e["batch"] == 2 and e["size"] in (224, 232)]


@pytest.fixture(scope="module")
def params():
    return W.make_densenet121_weights(0)


@pytest.mark.parametrize("entry", ENTRIES, ids=entry_id)
def test_launched_families_equal_the_fixture(params, monkeypatch, entry):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in entry["env"].items():
        monkeypatch.setenv(k, v)
    size, batch = entry["size"], entry["batch"]
    enc = DenseNet121Features(params, size, max_batch=batch, exact_weights=bool(entry["flags"] & 1))       # (the switches are read at create)
    stats, _ = enc.profile(torch.from_numpy(W.synthetic_frames_u8(batch, size)).cuda())
    assert [[s["name"], s["launches"], s["flops"], s["bytes"]] for s in stats] == entry["families"]
