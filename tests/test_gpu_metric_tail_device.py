"""The whole metric tail of the reference's test() on the device (`harness.evaluate_scores_device`: `iefvad_auc_ap` for the global
pair, two `iefvad_auc_ap_grouped` calls for the per-class pairs and the Ano-AUC) against the host tail (`harness.evaluate_scores`:
the sklearn calls of test.py:155-175): same numbers to 1e-12, same dict, same printed lines; and `harness.test(metric_tail="device")`
against the default call on the same scores.  `-m gpu`."""
import argparse

import numpy as np
import pytest
import torch

import iefvad_amd
from iefvad_amd import harness, synth

pytestmark = pytest.mark.gpu

QUIET = "Arrest"            # an abnormal class without a positive frame: the skip rule of test.py:168 runs


def make_list(keys, seed, quiet=None):
    """16 videos of synth.CONFIG1_LENGTHS over `keys` (every key at least once), sigmoid-like fp32 scores with ties, frame-level gt
    from synth.make_gt, the frames of class `quiet` cleared."""
    rng = np.random.default_rng(seed)
    lengths = synth.CONFIG1_LENGTHS
    classes = [keys[i % len(keys)] for i in range(len(lengths))]
    scores = [(np.round(1.0 / (1.0 + np.exp(-3.0 * rng.standard_normal(n))) * 4000) / 4000).astype(np.float32) for n in lengths]
    gt = synth.make_gt(seed, sum(lengths))
    st = 0
    for n, c in zip(lengths, classes):
        if c == quiet:
            gt[16 * st:16 * (st + n)] = 0.0
        st += n
    return scores, classes, gt


def assert_same_result(dev, host):
    for k in ("roc", "ap", "ano_auc"):
        assert abs(dev[k] - host[k]) < 1e-12, (k, dev[k] - host[k])
    assert list(dev["per_class"]) == list(host["per_class"])
    for c, (r, a) in host["per_class"].items():
        assert abs(dev["per_class"][c][0] - r) < 1e-12 and abs(dev["per_class"][c][1] - a) < 1e-12, c


@pytest.mark.parametrize("total_samples", [False, True])
def test_device_tail_equals_host_tail_on_a_ucf_list(capsys, total_samples):
    keys = harness.CLASS_KEYS["ucfcrime"]
    scores, classes, gt = make_list(keys, 21, quiet=QUIET)
    assert set(classes) == set(keys)
    host_log, dev_log = [], []
    host = harness.evaluate_scores(scores, classes, gt, "ucfcrime", total_samples=total_samples, log=host_log.append)
    host_out = capsys.readouterr().out
    dev = harness.evaluate_scores_device(scores, classes, gt, "ucfcrime", total_samples=total_samples, log=dev_log.append)
    dev_out = capsys.readouterr().out
    assert_same_result(dev, host)
    assert QUIET not in host["per_class"] and len(host["per_class"]) == len(keys) - 1
    assert dev_out.splitlines() == host_out.splitlines() and len(host_out.splitlines()) == 2 + 13 + 1
    assert ("Total Samples:" in host_out) == total_samples
    assert [list(d) for d in dev_log] == [list(d) for d in host_log]
    # one device tensor plus the per-video lengths, gt already on the device: the same numbers
    flat = torch.from_numpy(np.concatenate(scores)).cuda()
    dev2 = harness.evaluate_scores_device((flat, [len(s) for s in scores]), classes, torch.from_numpy(gt).cuda(), "ucfcrime", verbose=False)
    assert capsys.readouterr().out == ""
    assert dev2 == dev


def test_device_tail_on_the_xd_key_set(capsys):
    keys = harness.CLASS_KEYS["xd"]
    scores, classes, gt = make_list(keys, 22, quiet="riot")
    host = harness.evaluate_scores(scores, classes, gt, "xd", normal_keys=("normal",))
    host_out = capsys.readouterr().out
    dev = harness.evaluate_scores_device(scores, classes, gt, "xd", normal_keys=("normal",))
    assert capsys.readouterr().out.splitlines() == host_out.splitlines()
    assert_same_result(dev, host)
    assert "riot" not in dev["per_class"] and "normal" in dev["per_class"]
    # another Ano-AUC filter changes the Ano-AUC alone, in both
    host2 = harness.evaluate_scores(scores, classes, gt, "xd", verbose=False, normal_keys=("Normal",))
    dev2 = harness.evaluate_scores_device(scores, classes, gt, "xd", verbose=False, normal_keys=("Normal",))
    assert_same_result(dev2, host2)
    assert host2["ano_auc"] != host["ano_auc"]


def test_a_key_without_a_video_raises_in_both(capsys):
    keys = harness.CLASS_KEYS["ucfcrime"]
    scores, classes, gt = make_list(keys, 23)
    classes = ["Abuse" if c == "Vandalism" else c for c in classes]
    with pytest.raises(ValueError):
        harness.evaluate_scores(scores, classes, gt, "ucfcrime")
    with pytest.raises(ValueError):
        harness.evaluate_scores_device(scores, classes, gt, "ucfcrime")
    capsys.readouterr()


def test_harness_test_with_the_device_tail(tmp_path, capsys):
    """harness.test on a small model (one layer, one refinement step, a list of a few chunks): metric_tail="device" returns what the
    default call returns on the same scores, prints the same lines and leaves the same `last_result` otherwise."""
    keys = harness.CLASS_KEYS["ucfcrime"]
    lengths = [37, 100, 255, 256, 257, 64, 129, 16, 1, 90, 20, 50, 70, 33, 5, 12]
    classes = [keys[i % len(keys)] for i in range(len(lengths))]
    rows = []
    for i, (n, c) in enumerate(zip(lengths, classes)):
        img, ev = synth.make_video(31, i, n)
        d = tmp_path / "rgb" / c
        d.mkdir(parents=True, exist_ok=True)
        (tmp_path / "event_thr_10" / c).mkdir(parents=True, exist_ok=True)
        p = str(d / f"v{i:03d}__5.npy")
        np.save(p, img)
        np.save(p.replace("rgb", "event_thr_10"), ev)
        rows.append((p, c))
    csv = tmp_path / "test.csv"
    csv.write_text("path,label\n" + "".join(f"{p},{c}\n" for p, c in rows))
    gt = synth.make_gt(31, sum(lengths))
    st = 0
    for n, c in zip(lengths, classes):
        if c == QUIET:
            gt[16 * st:16 * (st + n)] = 0.0
        st += n
    args = argparse.Namespace(dataset="ucfcrime", visual_length=256, test_list=str(csv), exp_name="t", visual_layers=1, visual_head=8,
                              num_refinement_steps=1, lambda_ref=0.5, noise_model="StudentT", nu=8)
    model = iefvad_amd.MMFMIL(14, 768, 256, 768, 8, 1, 8, 10, 10, "cuda", args, compute="f32")
    model.load_state_dict(synth.make_state_dict(5, 768, 1, 1))
    with pytest.raises(ValueError, match="metric_tail"):
        harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", metric_tail="gpu")
    ret_host = harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0")
    host = harness.test.last_result
    host_out = capsys.readouterr().out
    ret_dev = harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", metric_tail="device")
    dev = harness.test.last_result
    assert capsys.readouterr().out.splitlines() == host_out.splitlines()
    assert sorted(dev) == sorted(host) and dev["classes"] == host["classes"] == classes
    for k in ("scores", "w_i_mean", "w_e_mean"):
        assert all(np.array_equal(a, b) for a, b in zip(dev[k], host[k])) and len(dev[k]) == len(lengths)
    assert_same_result(dev, host)
    assert abs(ret_dev[0] - ret_host[0]) < 1e-12 and abs(ret_dev[1] - ret_host[1]) < 1e-12
    assert QUIET not in dev["per_class"] and len(dev["per_class"]) == 13
    # the per-video pattern leaves gaps between the videos' scores on the device: the device tail takes the valid snippets only
    harness.test(args, model, harness.get_test_loader(args), 256, None, gt, "cuda:0", batch_chunks=0, metric_tail="device")
    capsys.readouterr()
    assert_same_result(harness.test.last_result, host)
