"""What swt_mlm_predict16 refuses from its arguments alone: SWT_ERR_INVALID naming the argument, before a device is looked for."""
import numpy as np
import pytest

ROWS, WIDTH, VOCAB, NPOS, K = 2, 3, 9, 2, 2
CASES = [("dtype:", {"dtype": 3}), ("dtype:", {"dtype": 0}), ("logits is not aligned", {"logits": 1}), ("k is above", {"k": 65}),
         ("k: out_top_id", {"k": 0}), ("labels: out_label_id", {"labels": None})]


@pytest.mark.parametrize("word, over", CASES)
def test_host_form_refuses_bad_arguments_without_a_device(native, word, over):
    """an unknown dtype, logits off their 2-byte alignment, k above 64, top outputs with k == 0, label outputs without labels"""
    a = {"logits": np.zeros(ROWS * WIDTH * VOCAB, np.uint16), "pos": np.arange(NPOS, dtype=np.uint64), "labels": np.zeros(ROWS * WIDTH, np.int32),
         "out_lse": np.zeros(NPOS, np.float32), "out_top_id": np.zeros(NPOS * K, np.int32), "out_top_logit": np.zeros(NPOS * K, np.float32),
         "out_label_id": np.zeros(NPOS, np.int32), "out_label_logit": np.zeros(NPOS, np.float32), "out_label_rank": np.zeros(NPOS, np.int32),
         "info": np.zeros(5, np.uint64)}
    v = {"dtype": native.FILL_BF16, "k": K}
    v.update({name: arr.ctypes.data for name, arr in a.items()})
    v.update({name: (v[name] + x if name == "logits" else x) for name, x in over.items()})
    lib = native.lib()
    rc = lib.swt_mlm_predict16(v["logits"], v["dtype"], ROWS, WIDTH, VOCAB, v["pos"], NPOS, v["labels"], 0, v["k"], v["out_lse"], v["out_top_id"],
                               v["out_top_logit"], v["out_label_id"], v["out_label_logit"], v["out_label_rank"], v["info"])
    assert rc == native.ERR_INVALID and word in lib.swt_last_error().decode(), lib.swt_last_error().decode()
