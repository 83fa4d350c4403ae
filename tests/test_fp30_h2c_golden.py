"""CPU: tests/golden/h2c_g2_fp30.json, the record of bls_py.hash_to_g2 that tests/test_gpu_fp30_chain.py compares the
device's G2 hash with (the pure-Python oracle takes 0.4 s a point, too long for 70 points in the GPU suite). The record
must hold exactly the messages that test generates, and a sample of its points (the empty message, the longest, one
of the partial wave) is derived again here. `python tests/test_fp30_h2c_golden.py` writes the record anew."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def _gpu_module():
    spec = importlib.util.spec_from_file_location("gpu_fp30_chain", os.path.join(ROOT, "tests", "test_gpu_fp30_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_record_matches_messages_and_oracle_sample():
    import bls_py as b
    t = _gpu_module()
    msgs = t.messages(t.SEED_G2, t.N_G2)
    with open(t.GOLDEN_G2) as f:
        rec = json.load(f)
    assert rec["dst"] == b.DST_G2.decode()
    assert rec["messages"] == [m.hex() for m in msgs]
    assert len(rec["hash_to_g2"]) == t.N_G2
    assert len(msgs[0]) == 0 and len(msgs[14]) == 200
    for i in (0, 14, 67):
        assert rec["hash_to_g2"][i] == b.g2_compress(b.hash_to_g2(msgs[i], b.DST_G2)).hex(), i


if __name__ == "__main__":
    import bls_py as b
    t = _gpu_module()
    msgs = t.messages(t.SEED_G2, t.N_G2)
    rec = {"dst": b.DST_G2.decode(), "messages": [m.hex() for m in msgs],
           "hash_to_g2": [b.g2_compress(b.hash_to_g2(m, b.DST_G2)).hex() for m in msgs]}
    with open(t.GOLDEN_G2, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
