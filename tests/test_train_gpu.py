"""GPU: kb.training.train against what the reference's train() recorded on the same inputs (tests/golden/train_kitti_narrow.npz,
written by tests/golden/gen_train_golden.py), against the hand-written loop of INTEGRATION.md bit for bit, and kb.summary.EventWriter
end to end: the event files of a run read back by the reader of tests/event_cases.py.

    python -m pytest tests/test_train_gpu.py -m gpu -q -s

Three runs of three steps on three 24 x 40 frames, shared through module fixtures: train() with the default writers, train() with
recording writers, the manual loop with recording writers that keep the tensors."""
import math
import os
import re
import shutil

import numpy as np
import pytest
import torch

import kbnet_amd as kb
import event_cases as ec
import run_cases as rc
import train_cases as tc

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4      # the package's bar for the loss against the reference (tests/test_loss_gpu.py, TOL)
STEP = r"^Step=\s+(\d+)/3  Loss=\d+\.\d{5}  Time Elapsed=\d+\.\d{2}h  Time Remaining=\d+\.\d{2}h$"
NUMBERS = r"^\s+(\d+)(\s+\d+\.\d{3}){4}$"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(tc.GOLDEN)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The four path lists, the depth checkpoint and the pose checkpoint (rebuilt from the generator's seed) in one directory."""
    root = tmp_path_factory.mktemp("train_inputs")

    def write_paths(filepath, paths):
        with open(filepath, "w") as f:
            f.write("\n".join(paths) + "\n")

    lists = [str(root / name) for name in rc.write_lists(str(root), write_paths)]
    depth = shutil.copy(rc.CHECKPOINT, str(root))
    pose = str(root / tc.POSE_CHECKPOINT)
    tc.write_pose_checkpoint(kb, pose)
    return {"lists": lists, "depth": depth, "pose": pose, "settings": tc.train_settings(kb.kitti_config().narrow())}


def _seed():
    torch.manual_seed(0)
    np.random.seed(0)


def _train(inputs, out, **more):
    lists = inputs["lists"]
    _seed()
    return kb.training.train(lists[0], lists[1], lists[2], lists[0], lists[1], lists[2], lists[3], checkpoint_path=out,
                             depth_model_restore_path=inputs["depth"], pose_model_restore_path=inputs["pose"], device="cuda",
                             workers=2, return_results=True, **inputs["settings"], **more)


def _final_parameters(out, step):
    depth = torch.load(os.path.join(out, f"depth_model-{step}.pth"), map_location="cpu")
    pose = torch.load(os.path.join(out, f"pose_model-{step}.pth"), map_location="cpu")
    tensors = {}
    for ckpt, keys in ((depth, ("sparse_to_dense_pool_state_dict", "encoder_state_dict", "decoder_state_dict")),
                       (pose, ("encoder_state_dict", "decoder_state_dict"))):
        for key in keys:
            for name, t in ckpt[key].items():
                tensors[f"{'pose' if ckpt is pose else 'depth'}.{key}.{name}"] = t
    return tensors


@pytest.fixture(scope="module")
def default_run(dev, inputs, tmp_path_factory):
    """train() with the default summary_writer_factory: the event files."""
    out = str(tmp_path_factory.mktemp("train_default") / "trained")
    results, logged, checkpoints = _train(inputs, out)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints}


@pytest.fixture(scope="module")
def recorded_run(dev, inputs, tmp_path_factory):
    """train() with recording writers: the call lists."""
    out = str(tmp_path_factory.mktemp("train_recorded") / "trained")
    writers = []

    def factory(log_dir):
        writers.append(tc.RecordingWriter(log_dir))
        return writers[-1]

    results, logged, checkpoints = _train(inputs, out, summary_writer_factory=factory)
    return {"out": out, "results": results, "logged": logged, "checkpoints": checkpoints, "writers": writers}


@pytest.fixture(scope="module")
def manual_run(dev, inputs, tmp_path_factory):
    """The hand-written loop of INTEGRATION.md ('The training iteration') over the same classes, under the same seeds, its writers
    keeping every tensor handed to them."""
    out = str(tmp_path_factory.mktemp("train_manual") / "trained")
    os.makedirs(out)
    s = inputs["settings"]
    lists = [kb.loader.read_paths(p) for p in inputs["lists"]]
    _seed()
    device = torch.device("cuda")
    model_keys = ("input_channels_image", "input_channels_depth", "min_pool_sizes_sparse_to_dense_pool", "max_pool_sizes_sparse_to_dense_pool",
                  "n_convolution_sparse_to_dense_pool", "n_filter_sparse_to_dense_pool", "n_filters_encoder_image", "n_filters_encoder_depth",
                  "resolutions_backprojection", "n_filters_decoder", "deconv_type", "weight_initializer", "activation_func",
                  "min_predict_depth", "max_predict_depth")
    depth_model = kb.modules.KBNetModel(**{k: s[k] for k in model_keys}, device=device, trainable=True)
    depth_model.requires_grad_(True)
    pose_model = kb.modules.ResNetPoseNetModel(18, rotation_parameterization="axis", weight_initializer=s["weight_initializer"],
                                               activation_func="relu", device=device, trainable=True)
    pose_model.requires_grad_(True).set_batch_norm("batch")
    depth_model.restore_model(inputs["depth"])
    pose_model.restore_model(inputs["pose"])
    train_loader = kb.loader.TrainingFrameLoader(lists[0], lists[1], lists[2], shape=(s["n_height"], s["n_width"]),
                                                 random_crop_type=s["augmentation_random_crop_type"], batch_size=s["n_batch"], shuffle=True,
                                                 device=device, workers=2)
    train_transforms = kb.transforms.Transforms(normalized_image_range=s["normalized_image_range"],
                                                random_flip_type=s["augmentation_random_flip_type"],
                                                random_remove_points=s["augmentation_random_remove_points"],
                                                random_noise_type=s["augmentation_random_noise_type"],
                                                random_noise_spread=s["augmentation_random_noise_spread"])
    ground_truths = [np.stack(kb.loader.load_depth_with_validity_map(p), axis=-1) for p in lists[3]]
    val_dataloader = kb.loader.InferenceFrameLoader(lists[0], lists[1], lists[2], use_image_triplet=True, batch_size=1, device=device, workers=2)
    train_writer, val_writer = tc.RecordingWriter("train", keep=True), tc.RecordingWriter("val", keep=True)
    optimizer = kb.optim.Adam([{"params": depth_model.parameters(), "weight_decay": s["w_weight_decay_depth"]},
                               {"params": pose_model.parameters(), "weight_decay": s["w_weight_decay_pose"]}], lr=s["learning_rates"][0])
    best_results = {"step": -1, "mae": np.inf, "rmse": np.inf, "imae": np.inf, "irmse": np.inf}
    train_step, losses = 0, []
    log_path = os.path.join(out, "results.txt")
    for epoch in range(1, s["learning_schedule"][-1] + 1):
        if epoch == 2:      # learning_schedule [1, 3]: the second rate from the second epoch on
            for g in optimizer.param_groups:
                g["lr"] = s["learning_rates"][1]
        for image0, image1, image2, sparse_depth0, intrinsics in train_loader:
            train_step += 1
            image0, image1, image2, sparse_depth0, filtered_sparse_depth0, filtered_validity_map_depth0 = kb.transforms.train_inputs(
                train_transforms, image0, image1, image2, sparse_depth0, s["augmentation_probabilities"][0])
            output_depth0 = depth_model.forward(image0, sparse_depth0, filtered_validity_map_depth0, intrinsics)
            pose01 = pose_model.forward(image0, image1)
            pose02 = pose_model.forward(image0, image2)
            loss, loss_info = depth_model.compute_loss(
                image0=image0, image1=image1, image2=image2, output_depth0=output_depth0, sparse_depth0=filtered_sparse_depth0,
                validity_map_depth0=filtered_validity_map_depth0, intrinsics=intrinsics, pose01=pose01, pose02=pose02,
                w_color=s["w_color"], w_structure=s["w_structure"], w_sparse_depth=s["w_sparse_depth"], w_smoothness=s["w_smoothness"])
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            loss_info.pop("per_frame")
            depth_model.log_summary(summary_writer=train_writer, tag="train", step=train_step, image0=image0,
                                    image01=loss_info.pop("image01"), image02=loss_info.pop("image02"), output_depth0=output_depth0.detach(),
                                    sparse_depth0=filtered_sparse_depth0, validity_map0=filtered_validity_map_depth0, pose01=pose01,
                                    pose02=pose02, scalars=loss_info, n_display=min(s["n_batch"], s["n_summary_display"]))
            losses.append(loss.item())
            if train_step >= s["validation_start_step"]:
                best_results = kb.validation.validate(
                    depth_model=depth_model, dataloader=val_dataloader, ground_truths=ground_truths, step=train_step,
                    best_results=best_results, min_evaluate_depth=s["min_evaluate_depth"], max_evaluate_depth=s["max_evaluate_depth"],
                    device=device, summary_writer=val_writer, n_summary_display=s["n_summary_display"], log_path=log_path)
    depth_model.save_model(os.path.join(out, f"depth_model-{train_step}.pth"), train_step, optimizer)
    pose_model.save_model(os.path.join(out, f"pose_model-{train_step}.pth"), train_step, optimizer)
    return {"out": out, "losses": losses, "train_step": train_step, "best_results": best_results, "writers": (train_writer, val_writer)}


# ------------------------------------------------------------------------------------------------ text
def test_results_text_line_for_line(default_run, inputs, golden):
    with open(os.path.join(default_run["out"], "results.txt")) as f:
        got = f.read().splitlines()
    ref = str(golden["results"]).splitlines()
    assert len(got) == len(ref), ("\n".join(got), "\n".join(ref))
    path_lines = {1: 0, 2: 1, 3: 2, 6: 0, 7: 1, 8: 2, 9: 3}      # line -> list: the two path blocks
    assert ref[0] == "Training input paths:" and ref[5] == "Validation input paths:"
    steps = validations = 0
    for i, (g, r) in enumerate(zip(got, ref)):
        if i in path_lines:
            assert g == inputs["lists"][path_lines[i]] and os.path.basename(g) == r, (g, r)
        elif r.startswith(("checkpoint_path=", "event_path=", "depth_model_restore_path=", "pose_model_restore_path=")):
            key = r.split("=")[0] + "="
            assert g.startswith(key) and len(g) > len(key), (g, r)
        elif r.startswith("device="):
            assert (g, r) == ("device=cuda", "device=cpu")
        elif re.match(STEP, r):
            assert re.match(STEP, g) and re.match(STEP, g).group(1) == re.match(STEP, r).group(1), (g, r)
            steps += 1
        elif re.match(NUMBERS, r):
            assert re.match(NUMBERS, g), (g, r)
            if ref[i - 2] == "Validation results:":
                assert re.match(NUMBERS, g).group(1) == re.match(NUMBERS, r).group(1), (g, r)
                validations += 1
        else:
            assert g == r, (i, g, r)
    assert steps == 3 and validations == 2
    assert any(line == "event_path=" + os.path.join(default_run["out"], "events") for line in got)


# ------------------------------------------------------------------------------------------------ the writers' calls
def _calls(golden, which):
    return [(str(m), str(t), int(s)) for m, t, s in golden[which]]


def test_recording_writers_receive_the_references_calls(recorded_run, golden):
    train_writer, val_writer = recorded_run["writers"]
    assert train_writer.log_dir == os.path.join(recorded_run["out"], "events-train") and val_writer.log_dir == os.path.join(recorded_run["out"], "events-val")
    assert train_writer.calls == _calls(golden, "calls_train")
    assert val_writer.calls == _calls(golden, "calls_val")
    assert train_writer.closed == 1 and val_writer.closed == 1
    assert len(train_writer.calls) == 45 and len(val_writer.calls) == 16


def test_writers_are_closed_when_the_run_fails(dev, inputs, tmp_path):
    writers = []

    def factory(log_dir):
        writers.append(tc.RecordingWriter(log_dir))
        if len(writers) == 2:
            writers[-1].add_histogram = None      # the first log_summary of validate() fails
        return writers[-1]

    with pytest.raises(TypeError):
        _train(inputs, str(tmp_path / "trained"), summary_writer_factory=factory)
    assert [w.closed for w in writers] == [1, 1]


# ------------------------------------------------------------------------------------------------ checkpoints
def test_checkpoints(default_run, golden, dev):
    out = default_run["out"]
    names = sorted(n for n in os.listdir(out) if n.endswith(".pth"))
    assert names == [str(n) for n in golden["checkpoints"]]
    assert sorted(os.path.basename(p) for p in default_run["checkpoints"]) == names and len(default_run["checkpoints"]) == 6
    for name, step, lrs in zip(names, golden["checkpoint_steps"], golden["checkpoint_lrs"]):
        ckpt = torch.load(os.path.join(out, name), map_location="cpu")
        assert int(ckpt["train_step"]) == int(step), name
        assert [float(g["lr"]) for g in ckpt["optimizer_state_dict"]["param_groups"]] == [float(v) for v in lrs], name
    cfg = kb.kitti_config().narrow()
    depth_model = kb.modules.KBNetModel.from_config(cfg, device=dev)
    for step in (1, 2, 3):
        got_step, _ = depth_model.restore_model(os.path.join(out, f"depth_model-{step}.pth"))
        pose_model = kb.modules.load_pose_model(os.path.join(out, f"pose_model-{step}.pth"), device=dev, activation_func="relu")
        assert got_step == step and isinstance(pose_model, kb.modules.ResNetPoseNetModel) and pose_model.n_layer == 18
    assert default_run["results"]["train_step"] == 3 and default_run["results"]["best_results"]["step"] in (2, 3)


# ------------------------------------------------------------------------------------------------ numbers
def test_first_loss_against_the_reference(default_run, golden):
    """Step 1's loss, before any update, within 1e-4 relative of the reference's; the later steps are printed here and gated in
    tests/test_train_trajectory_gpu.py, against an fp64 restatement of the run and by what fp32 rounding alone does to it (a fixed
    bar cannot work past step 1: Adam's first steps amplify rounding, its update is lr * sign-like for every weight)."""
    want = golden["losses"]
    got = [value for _, value in default_run["logged"]]
    assert [step for step, _ in default_run["logged"]] == [1, 2, 3]
    for step, (g, w) in enumerate(zip(got, want), 1):
        print(f"step {step}: loss {g!r}, the reference's {w!r}, relative distance {abs(g - w) / abs(w):.3e}")
    assert abs(got[0] - want[0]) <= LOSS_TOL * abs(want[0])
    assert all(math.isfinite(g) for g in got)


def test_bit_equal_to_the_manual_loop(recorded_run, manual_run, default_run):
    """The same final parameters, bit for bit, and the same loss sequence as the hand-written loop under the same seeds."""
    assert [value for _, value in recorded_run["logged"]] == manual_run["losses"] == [value for _, value in default_run["logged"]]
    assert recorded_run["results"]["train_step"] == manual_run["train_step"] == 3
    assert recorded_run["results"]["best_results"] == manual_run["best_results"]
    want = _final_parameters(manual_run["out"], 3)
    for run in (recorded_run, default_run):
        got = _final_parameters(run["out"], 3)
        assert sorted(got) == sorted(want) and len(want) > 100
        differing = [k for k in want if not torch.equal(got[k], want[k])]
        assert not differing, differing[:5]
    # and the run moved: the parameters differ from the restored ones
    first = _final_parameters(recorded_run["out"], 1)
    assert sum(not torch.equal(first[k], want[k]) for k in want if want[k].is_floating_point()) > 100


# ------------------------------------------------------------------------------------------------ EventWriter end to end
@pytest.mark.parametrize("which", ["train", "val"])
def test_event_files_of_a_run(default_run, manual_run, golden, which):
    directory = os.path.join(default_run["out"], "events-" + which)
    files = os.listdir(directory)
    assert len(files) == 1 and files[0].startswith("events.out.tfevents.")
    events = ec.read_events(os.path.join(directory, files[0]))      # both checksums of every record
    assert events[0]["file_version"] == "brain.Event:2"
    kinds = {"add_scalar": "scalar", "add_histogram": "histo", "add_image": "image"}
    calls = _calls(golden, "calls_" + which)
    assert [(e["kind"], e["tag"], e["step"]) for e in events[1:]] == [(kinds[m], t, s) for m, t, s in calls]
    writer = manual_run["writers"][0 if which == "train" else 1]
    assert writer.calls == calls
    edges = ec.tensorflow_edges()
    seen = {"scalar": 0, "histo": 0, "image": 0}
    for e, value in zip(events[1:], writer.tensors):
        seen[e["kind"]] += 1
        if e["kind"] == "scalar":
            want = value.item() if torch.is_tensor(value) else value
            assert e["value"] == float(np.float32(want)), e["tag"]
        elif e["kind"] == "histo":
            x = value.detach().cpu().numpy().astype(np.float32)
            limits, counts = ec.make_histogram_oracle(ec.histogram_oracle(x, edges), edges)
            lo, hi, num, total, squares, bound_total, bound_squares = ec.stats_oracle(x)
            h = e["value"]
            assert np.array_equal(h["bucket_limit"], limits) and np.array_equal(h["bucket"], counts.astype(np.float64)), e["tag"]
            assert (h["min"], h["max"], h["num"]) == (lo, hi, num), e["tag"]
            assert abs(h["sum"] - total) <= bound_total and abs(h["sum_squares"] - squares) <= bound_squares, e["tag"]
        else:
            height, width, colorspace, png = e["value"]
            panel = value.detach().cpu().numpy()
            assert (colorspace, height, width) == tuple(panel.shape), e["tag"]
            assert np.array_equal(kb.loader.decode_png(png), rc.oracle_rgb(panel[None], 255.0, 0.0)[0]), e["tag"]
    assert all(seen.values()), seen
