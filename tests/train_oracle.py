"""One training run of kb.training.train, restated on the CPU in any dtype: test infrastructure, never imported by the package.

The existing oracles composed into train()'s iteration:

    inputs   the three frames of run_cases.path_lists() as ONE batch, made as train() makes them: load_image_triplet's split and
             order, / 255; the raw sparse depth; pre_eval_cases.outlier_removal(., 7, 1.5) for the filtered pair; augmentation off
    state    ckpt_kitti_narrow.pth (depth) and kb.synthetic.make_resnet_pose_weights(18, seed=POSE_SEED) (pose)
    a step   kbnet_grad_oracle.forward(image0, RAW sparse depth, filtered validity, intrinsics)
             resnet_pose_grad_oracle.forward(batch_norm='batch') on (image0, image1), then on (image0, image2): each writes its
             running statistics back before the next
             loss_oracle.pose_matrix, compute_loss on the FILTERED pair with the run's four weights
             torch.autograd through all of it
             adam_oracle's formula (`adam_update`: one step of it, resumable) over two groups, weight decay 0 / 1e-4, scheduled rate
    probes   the networks as functions after the step: the depth output on the frames in validation order with
             pre_eval_cases.eval_oracle's metrics (what validate() logs), the pose six-vectors of both pairs in running-statistics
             mode (what a restored checkpoint computes), the running statistics themselves

fp64 is the yardstick; fp32 (torch's CPU kernels) measures what rounding alone does to a trajectory.  `run(..., start=state)`
resumes from any state -- a device checkpoint included -- which is what the teacher-forced comparison needs: one oracle step
from the state the run under test left.  MISTAKES are planted for the power test (tests/test_train_oracle_cpu.py)."""
import math
import os
import re

import numpy as np
import torch

import kbnet_amd as kb
import adam_oracle as ao
import kbnet_grad_oracle as kgo
import loss_oracle as lo
import posenet_grad_oracle as pgo
import pre_eval_cases as pec
import resnet_pose_grad_oracle as rpgo
import run_cases as rc
import train_cases as tc

GOLDEN = os.path.join(rc.GOLDEN_DIR, "train_trajectory_kitti_narrow.npz")
N_STEPS = 8
LEARNING_RATES, LEARNING_SCHEDULE = [1e-4, 5e-5], [3, N_STEPS]      # the rate changes at step 4, away from Adam's special first step
VALIDATION_START_STEP = 2
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
POSE_SLOPE = 0.0      # train() builds the pose network with activation_func='relu'
METRICS = ("mae", "rmse", "imae", "irmse")

MISTAKES = ("lr_change_ignored", "lr_change_one_step_late", "adam_step_not_carried", "moments_reset_each_step", "stale_depth_weights",
            "stale_pose_weights", "second_pose_forward_leaves_running_stats", "biased_running_var", "weight_decay_on_depth_group",
            "pose_eval_mode_after_validation")


def trajectory_settings(cfg):
    """train()'s keyword arguments of the eight-step run: train_cases.train_settings with eight epochs of one step and the rate
    changing after the third."""
    settings = tc.train_settings(cfg)
    settings.update(learning_rates=list(LEARNING_RATES), learning_schedule=list(LEARNING_SCHEDULE),
                    validation_start_step=VALIDATION_START_STEP, n_checkpoint=1)
    return settings


def learning_rate(step, mistake=None):
    """The rate of (1-based) step `step`: one step an epoch, kb.training.scheduled's rule."""
    if mistake == "lr_change_ignored":
        return LEARNING_RATES[0]
    if mistake == "lr_change_one_step_late":
        step = max(step - 1, 1)
    position = 0
    for epoch in range(1, step + 1):
        if epoch > LEARNING_SCHEDULE[position]:
            position += 1
    return LEARNING_RATES[position]


ROW = r"^\s+(\d+)\s+(\d+\.\d{3})\s+(\d+\.\d{3})\s+(\d+\.\d{3})\s+(\d+\.\d{3})$"


def validation_rows(text):
    """The number rows that follow 'Validation results:' and its header in a results.txt -> K x 5 float64: step, MAE, RMSE, iMAE,
    iRMSE."""
    lines = text.splitlines()
    rows = [[float(x) for x in re.match(ROW, lines[i + 2]).groups()] for i, line in enumerate(lines) if line == "Validation results:"]
    return np.asarray(rows, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def load_frames():
    """The frames as train()'s loader reads them, fp32 NumPy in list order: image0 / image1 / image2 in 0..255 (N x 3 x H x W), the
    raw sparse depth (N x 1 x H x W), the intrinsics (N x 3 x 3) and the validation ground truth with its validity (N x H x W each)."""
    image_paths, sparse_paths, intrinsics_paths, ground_truth_paths = rc.path_lists()
    triplets = [kb.loader.load_image_triplet(p, normalize=False) for p in image_paths]      # (t - 1, t, t + 1)
    truths = [kb.loader.load_depth_with_validity_map(p) for p in ground_truth_paths]
    return {"image0": np.stack([t[1] for t in triplets]), "image1": np.stack([t[0] for t in triplets]),
            "image2": np.stack([t[2] for t in triplets]),
            "sparse": np.stack([kb.loader.load_depth(p, data_format="CHW") for p in sparse_paths]),
            "intrinsics": np.stack([np.load(p).astype(np.float32) for p in intrinsics_paths]),
            "ground_truth": np.stack([t[0] for t in truths]), "ground_truth_validity": np.stack([t[1] for t in truths])}


_FRAMES = {}


LAYOUTS = ("contiguous", "channels_last")      # of the three images in memory: torch's fp32 CPU convolutions take another path for each


def batch(dtype, frame_order=(0, 1, 2), layout="contiguous"):
    """The tensors of one training batch in `dtype`, frames in `frame_order`: image0, image1, image2 (/ 255), sparse (raw),
    filtered_sparse, filtered_validity, intrinsics.  `layout`: the images' memory format -- the values are the same, the order in
    which an fp32 kernel sums them is not (a second set of fp32 runs for the yardsticks)."""
    assert layout in LAYOUTS, layout
    if not _FRAMES:
        _FRAMES.update(load_frames())
    order = list(frame_order)
    sparse = _FRAMES["sparse"][order]
    filtered_sparse, filtered_validity = pec.outlier_removal(sparse, 7, 1.5)      # over the batch, as train_inputs
    out = {k: torch.from_numpy(np.ascontiguousarray(_FRAMES[k][order])).to(dtype) / 255.0 for k in ("image0", "image1", "image2")}
    out.update(sparse=torch.from_numpy(sparse).to(dtype), filtered_sparse=torch.from_numpy(filtered_sparse).to(dtype),
               filtered_validity=torch.from_numpy(filtered_validity).to(dtype),
               intrinsics=torch.from_numpy(_FRAMES["intrinsics"][order]).to(dtype))
    if layout == "channels_last":
        out.update({k: out[k].contiguous(memory_format=torch.channels_last) for k in ("image0", "image1", "image2")})
    return out


def ground_truths():
    """(depth, validity) of the validation ground truths, N x H x W fp32 NumPy each, in list order."""
    if not _FRAMES:
        _FRAMES.update(load_frames())
    return _FRAMES["ground_truth"], _FRAMES["ground_truth_validity"]


# ------------------------------------------------------------------------------------------------ state
DEPTH_GROUPS = (("s2d", "sparse_to_dense_pool_state_dict"), ("enc", "encoder_state_dict"), ("dec", "decoder_state_dict"))
POSE_GROUPS = (("enc", "encoder_state_dict"), ("dec", "decoder_state_dict"))


def is_running(key):
    return key.endswith(("running_mean", "running_var", "num_batches_tracked"))


def state_from_checkpoints(depth_ckpt, pose_ckpt, dtype, step=0, with_optimizer=True):
    """A state from the two checkpoint dicts of a step (the reference's layout, as train() restores and writes it): 'depth' and
    'pose' (name -> parameter, '<group>::<key>' in the optimizer's order), 'running' (the pose BatchNorm buffers), 'm', 'v', 'count'
    (Adam's state by parameter name; a parameter that never had a gradient has none and count 0), 'lr' (the rates in the
    checkpoint, None without an optimizer state) and 'step' (the steps taken)."""
    depth, pose, running = {}, {}, {}
    for grp, key in DEPTH_GROUPS:
        for k, v in pgo.po.strip(depth_ckpt[key]).items():
            depth[f"{grp}::{k}"] = v.detach().cpu().to(dtype)
    for grp, key in POSE_GROUPS:
        for k, v in pgo.po.strip(pose_ckpt[key]).items():
            v = v.detach().cpu()
            if is_running(k):
                running[f"{grp}::{k}"] = v.to(dtype) if v.is_floating_point() else v.clone()
            else:
                pose[f"{grp}::{k}"] = v.to(dtype)
    state = {"depth": depth, "pose": pose, "running": running, "m": {}, "v": {}, "count": {k: 0 for k in list(depth) + list(pose)},
             "lr": None, "step": int(step)}
    optimizer = (depth_ckpt.get("optimizer_state_dict") or {}) if with_optimizer else {}      # train() restores the weights alone
    if optimizer:
        groups = optimizer["param_groups"]
        names = [list(depth), list(pose)]
        assert [len(g["params"]) for g in groups] == [len(n) for n in names], ([len(g["params"]) for g in groups], [len(n) for n in names])
        state["lr"] = [float(g["lr"]) for g in groups]
        for group, group_names in zip(groups, names):
            for index, name in zip(group["params"], group_names):
                entry = optimizer["state"].get(index)
                if entry is not None:
                    assert entry["exp_avg"].shape == (depth if name in depth else pose)[name].shape, name      # the order is the optimizer's
                    state["m"][name] = entry["exp_avg"].detach().cpu().to(dtype)
                    state["v"][name] = entry["exp_avg_sq"].detach().cpu().to(dtype)
                    state["count"][name] = int(float(entry["step"]))
    return state


def initial_state(dtype):
    """What train() restores: the committed depth checkpoint and the seeded pose weights."""
    depth_ckpt = torch.load(rc.CHECKPOINT, map_location="cpu")
    enc, dec = kb.synthetic.make_resnet_pose_weights(18, seed=tc.POSE_SEED)
    return state_from_checkpoints(depth_ckpt, {"encoder_state_dict": enc, "decoder_state_dict": dec}, dtype, with_optimizer=False)


def cast_state(state, dtype):
    """`state` with every floating tensor in `dtype` (the integer counts as they are): the start of a teacher-forced step."""
    def cast(d):
        return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
    out = dict(state)
    for key in ("depth", "pose", "running", "m", "v"):
        out[key] = cast(state[key])
    for key in ("stale_depth", "stale_pose"):
        out.pop(key, None)
    return out


def _split(named, groups):
    return [{k[len(g) + 2:]: v for k, v in named.items() if k.startswith(g + "::")} for g in groups]


def pose_state_dicts(pose, running):
    """(encoder, decoder) state dicts of the pose network from a state's 'pose' and 'running'."""
    merged = dict(pose)
    merged.update(running)
    return _split(merged, ("enc", "dec"))


# ------------------------------------------------------------------------------------------------ Adam, one step
def adam_update(p, g, m, v, count, lr, weight_decay, mistake=None):
    """adam_oracle.adam's formula for one parameter and one step, from any (m, v, count): -> (p, m, v, count).  Equal to it bit
    for bit over a sequence (tests/test_train_oracle_cpu.py)."""
    beta1, beta2 = BETAS
    if m is None or mistake == "moments_reset_each_step":
        m, v = torch.zeros_like(p), torch.zeros_like(p)
    count = count + 1
    t = 1 if mistake == "adam_step_not_carried" else count
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (1 - beta1) * (g - m)
    v = beta2 * v + (1 - beta2) * g * g
    step_size = lr / (1 - beta1 ** t)
    denom = torch.sqrt(v) / math.sqrt(1 - beta2 ** t) + ADAM_EPS
    return p - step_size * m / denom, m, v, count


# ------------------------------------------------------------------------------------------------ probes
def probes(state, cfg, dtype, layout="contiguous"):
    """The networks of `state` as functions, on the frames in VALIDATION order: 'depth' (N x 1 x H x W), 'metrics' (the four means
    over the frames of eval_oracle's rows: validate()'s logged row), 'metrics_per_frame', 'dof01' / 'dof02' (N x 6, BatchNorm on the
    running statistics)."""
    b = batch(dtype, layout=layout)
    with torch.no_grad():
        depth = kgo.forward(b["image0"], b["sparse"], b["filtered_validity"], b["intrinsics"], *_split(state["depth"], ("s2d", "enc", "dec")),
                            cfg)["depth"]
        enc, dec = pose_state_dicts(state["pose"], state["running"])
        dofs = [rpgo.forward(b["image0"], b[other], enc, dec, 18, batch_norm="running", slope=POSE_SLOPE)["dof"]
                for other in ("image1", "image2")]
    truth, validity = ground_truths()
    rows, _ = pec.eval_oracle(depth.float().numpy(), truth, validity, 0.0, 100.0)
    return {"depth": depth, "metrics": rows.mean(axis=0), "metrics_per_frame": rows, "dof01": dofs[0], "dof02": dofs[1]}


# ------------------------------------------------------------------------------------------------ the run
def step(state, b, cfg, dtype, mistake=None, weights=None):
    """One iteration of train() from `state` on the batch `b` -> (new state, record).  `weights`: the loss's four."""
    weights = weights or dict(w_color=0.15, w_structure=0.95, w_sparse_depth=0.60, w_smoothness=0.04)
    number = state["step"] + 1
    # the weights the FORWARD reads (and the gradient is taken at): the current ones, or with a planted stale cache the decoder's /
    # the pose encoder's of the step before; the update is applied to the current ones either way
    depth, pose = dict(state["depth"]), dict(state["pose"])
    if mistake == "stale_depth_weights" and "stale_depth" in state:
        depth.update({k: v for k, v in state["stale_depth"].items() if k.startswith("dec::")})
    if mistake == "stale_pose_weights" and "stale_pose" in state:
        pose.update({k: v for k, v in state["stale_pose"].items() if k.startswith("enc::")})
    forward_depth = {k: v.detach().clone().requires_grad_(True) for k, v in depth.items()}
    forward_pose = {k: v.detach().clone().requires_grad_(True) for k, v in pose.items()}
    running = dict(state["running"])
    pose_mode = "batch"
    if mistake == "pose_eval_mode_after_validation" and number > VALIDATION_START_STEP:
        pose_mode = "running"

    output_depth = kgo.forward(b["image0"], b["sparse"], b["filtered_validity"], b["intrinsics"],
                               *_split(forward_depth, ("s2d", "enc", "dec")), cfg)["depth"]
    dofs = []
    for index, other in enumerate(("image1", "image2")):
        enc, dec = pose_state_dicts(forward_pose, running)
        out = rpgo.forward(b["image0"], b[other], enc, dec, 18, batch_norm=pose_mode, slope=POSE_SLOPE,
                           biased_running_var=mistake == "biased_running_var")
        if not (index == 1 and mistake == "second_pose_forward_leaves_running_stats"):
            running = dict(out["running"])      # written back before the next forward reads them
        dofs.append(out["dof"])
    loss = lo.compute_loss(b["image0"], b["image1"], b["image2"], output_depth, b["filtered_sparse"], b["filtered_validity"],
                           b["intrinsics"], lo.pose_matrix(dofs[0]), lo.pose_matrix(dofs[1]), **weights)
    names = list(forward_depth) + list(forward_pose)
    leaves = list(forward_depth.values()) + list(forward_pose.values())
    grads = dict(zip(names, torch.autograd.grad(loss["loss"], leaves, allow_unused=True)))

    lr = learning_rate(number, mistake)
    decay = {"depth": 0.0, "pose": 1e-4}
    if mistake == "weight_decay_on_depth_group":
        decay = {"depth": 1e-4, "pose": 0.0}
    new = {"depth": {}, "pose": {}, "running": running, "m": {}, "v": {}, "count": {}, "lr": [lr, lr], "step": number,
           "stale_depth": state["depth"], "stale_pose": state["pose"]}
    for which in ("depth", "pose"):
        for name, p in state[which].items():
            g = grads[name]
            if g is None:      # never used by the forward: left alone, its step count too
                new[which][name], new["count"][name] = p, state["count"][name]
                if name in state["m"]:
                    new["m"][name], new["v"][name] = state["m"][name], state["v"][name]
                continue
            new[which][name], new["m"][name], new["v"][name], new["count"][name] = adam_update(
                p, g.detach(), state["m"].get(name), state["v"].get(name), state["count"][name], lr, decay[which], mistake)
    record = {"step": number, "loss": float(loss["loss"].detach()), "lr": lr,
              "terms": tuple(float(loss[k].detach()) for k in ("loss_color", "loss_structure", "loss_sparse_depth", "loss_smoothness")),
              "state": new, "dof01": dofs[0].detach(), "dof02": dofs[1].detach()}
    return new, record


def iterate(dtype, steps=N_STEPS, frame_order=(0, 1, 2), mistake=None, start=None, with_probes=True, layout="contiguous"):
    """The records of `steps` steps, one at a time (a record holds its whole state: a caller that keeps none keeps memory flat)."""
    assert mistake is None or mistake in MISTAKES, mistake
    cfg = kb.kitti_config().narrow()
    state = initial_state(dtype) if start is None else cast_state(start, dtype)
    b = batch(dtype, frame_order, layout)
    for _ in range(steps):
        state, record = step(state, b, cfg, dtype, mistake)
        if with_probes:
            record["probes"] = probes(state, cfg, dtype, layout)
        yield record


def run(dtype, steps=N_STEPS, frame_order=(0, 1, 2), mistake=None, start=None):
    """-> a list of one record a step: 'step', 'loss', 'terms' (colour, structure, sparse depth, smoothness), 'lr', 'state' (after
    the step: 'depth', 'pose', 'running' with num_batches_tracked, 'm', 'v', 'count', 'lr', 'step'), 'dof01' / 'dof02' (the step's
    own batch-mode six-vectors) and 'probes'.  `start`: a state to resume from (the index of the next step is its 'step' + 1)."""
    return list(iterate(dtype, steps, frame_order, mistake, start))


# ------------------------------------------------------------------------------------------------ distances
def _norm(pairs):
    return math.sqrt(sum(float((a.double() - b.double()).pow(2).sum()) for a, b in pairs))


def update_ratio(got, want, origin):
    """||got - want||_2 / ||want - origin||_2 over dicts of tensors with the same keys: the error against how far the run moved."""
    assert sorted(got) == sorted(want) == sorted(origin)
    moved = _norm((want[k], origin[k]) for k in want)
    return _norm((got[k], want[k]) for k in want) / moved if moved else float("inf")


def _floating(running):
    return {k: v for k, v in running.items() if v.is_floating_point()}


def relative(a, b):
    return abs(a - b) / abs(b)


def distances(got, want, origin):
    """Every distance of a state-and-probes record `got` from the record `want` (fp64), the updates measured from the state
    `origin` (the initial state of a free run, the state a teacher-forced step started from) -> dict of floats."""
    gs, ws = got["state"], want["state"]
    out = {"loss": relative(got["loss"], want["loss"]),
           "depth": update_ratio(gs["depth"], ws["depth"], origin["depth"]),
           "pose": update_ratio(gs["pose"], ws["pose"], origin["pose"]),
           "running": update_ratio(_floating(gs["running"]), _floating(ws["running"]), _floating(origin["running"]))}
    for which in ("depth", "pose"):      # Adam's moments by adam_oracle.fraction, the worst tensor of each network
        for moment in ("m", "v"):
            out[f"{moment}_{which}"] = max(ao.fraction(gs[moment][k], ws[moment][k]) for k in ws[moment] if k in ws[which])
    if "probes" in got and "probes" in want:
        gp, wp = got["probes"], want["probes"]
        out["probe_depth"] = pgo.fraction(gp["depth"], wp["depth"])
        out["probe_pose"] = max(pgo.fraction(gp[k], wp[k]) for k in ("dof01", "dof02"))
        for i, name in enumerate(METRICS):
            out[name] = relative(float(gp["metrics"][i]), float(wp["metrics"][i]))
    return out


DISTANCES = ("loss", "depth", "pose", "running", "m_depth", "v_depth", "m_pose", "v_pose", "probe_depth", "probe_pose") + METRICS


def exact_findings(got, want):
    """What must agree exactly between two states: Adam's step counts, num_batches_tracked, which parameters have moments."""
    findings = []
    for k, count in want["count"].items():
        if got["count"].get(k) != count:
            findings.append(f"step count of {k}: {got['count'].get(k)}, expected {count}")
    if sorted(got["m"]) != sorted(want["m"]):
        findings.append(f"moments exist for other parameters: {sorted(set(got['m']) ^ set(want['m']))[:4]}")
    for k, v in want["running"].items():
        if not v.is_floating_point() and int(got["running"][k]) != int(v):
            findings.append(f"{k}: {int(got['running'][k])}, expected {int(v)}")
    return findings


THREADS = 8      # of torch's CPU kernels while a yardstick is measured, the reference's run included: seven fp32 runs under one condition


def free_and_forced(frame_order, steps=N_STEPS, layout="contiguous"):
    """The fp32 oracle (its images in `layout`) against the fp64 oracle for one frame order -> (free, forced, own): per step, `distances` of the free-running
    fp32 run (updates from the initial state), of ONE fp32 step from the fp64 state of the step before (updates from that state), and
    of the free-running fp32 run's step against ONE fp64 step from ITS OWN state of the step before -- the form in which the device
    is measured (FORCED_GATES only: no probes).
    Measured with THREADS threads: how torch's CPU kernels split a sum follows the thread count, and a free-running fp32 trajectory
    amplifies the last bit (its loss distance at a late step moves between 3e-5 and 1e-3 with the count), so a figure reproduces
    only at the count it was taken with."""
    before = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    try:
        return _free_and_forced(frame_order, steps, layout)
    finally:
        torch.set_num_threads(before)


def _free_and_forced(frame_order, steps, layout):
    free, forced, own = [], [], []
    origin = initial_state(torch.float64)
    previous, previous32 = origin, origin
    for r32, r64 in zip(iterate(torch.float32, steps, frame_order, layout=layout), iterate(torch.float64, steps, frame_order)):
        free.append(distances(r32, r64, origin))
        one = next(iterate(torch.float32, 1, frame_order, start=previous, layout=layout))
        forced.append(distances(one, r64, previous))
        want = next(iterate(torch.float64, 1, frame_order, start=previous32, with_probes=False))
        own.append(distances(r32, want, cast_state(previous32, torch.float64)))
        previous, previous32 = r64["state"], r32["state"]
    return free, forced, own


def metric_floor(depth, tol=kgo.TOL):
    """What a forward inside its own bar, |d - d64| <= tol (|d64| + rms(d64)) per element (the depth network's gate, the device
    forward is not IEEE fp32), can move the four logged metrics by (absolute, in their units): with e = that bound per pixel,
    |MAE' - MAE| <= 1000 mean e, |RMSE' - RMSE| <= 1000 sqrt(mean e^2) (the triangle inequality in L2), and the same for the inverse
    metrics with e / (d (d - e)) [1/km] -- each over the frame's counted pixels, then the mean over the frames -> four numbers."""
    truth, validity = ground_truths()
    d = depth.detach().double().numpy().reshape(truth.shape)
    bounds = np.zeros((d.shape[0], 4))
    for i in range(d.shape[0]):
        mask = (validity[i] > 0) & (truth[i] > 0.0) & (truth[i] < 100.0)
        e = tol * (np.abs(d[i]) + np.sqrt((d[i] ** 2).mean()))
        ie = e / (d[i] * (d[i] - e))
        bounds[i] = [1000.0 * e[mask].mean(), 1000.0 * np.sqrt((e[mask] ** 2).mean()), 1000.0 * ie[mask].mean(),
                     1000.0 * np.sqrt((ie[mask] ** 2).mean())]
    return bounds.mean(axis=0)


# ------------------------------------------------------------------------------------------------ the gates
MARGIN = 3.0                # a gate is 3 x what fp32 rounding alone does to the same quantity
REFERENCE_MARGIN = 1.5      # the reference as a seventh fp32 run: room for an order of summation the six do not contain
LOSS_TOL = 1e-4             # the package's bar for the loss (tests/test_loss_gpu.py, tests/test_train_gpu.py)
FORCED_GATES = ("loss", "depth", "pose", "running", "m_depth", "v_depth", "m_pose", "v_pose")
FREE_GATES = ("loss", "depth", "running", "probe_depth", "probe_pose") + METRICS
FREE_DEPTH_STEPS = (4, 8)
# The teacher-forced gates of the parameters and of Adam's moments take their yardstick from the WORST of steps 2 .. 8, not from the
# step's own figure (step 1, Adam's sign-like first update, keeps its own).  Their one-step fp32 distance is decided by single
# activation decisions: on these frames the maps are 12 x 20 down to 1 x 1 over three frames, and one ReLU, leaky-ReLU or pool-window
# choice that fp32 and fp64 take differently moves a whole channel's gradient.  A step's figure is then 3e-5 or 4e-3 (the depth
# update ratio; 1e-5 or 3e-2 for the depth network's m) by the luck of the state it starts from -- and the six frame orders, stepped
# from the SAME fp64 state, are one draw a step, not six (the fixture's `forced`, equal over the orders to two digits).  The fp32
# oracle stepped from its OWN states, as the device is measured (the fixture's `forced_own`), leaves 3 x the step's own figure by
# factors of 30 to 350: a gate of that form fails an implementation that differs from fp64 by fp32 rounding alone
# (tests/test_train_oracle_cpu.py::test_fp32_oracle_measured_as_the_device_is).  The envelope is over both forms.  The loss and the
# running statistics, which no single decision moves, keep their per-step yardstick.  DESIGN section 8q has the device's figures.
ENVELOPE_GATES = ("depth", "pose", "m_depth", "v_depth", "m_pose", "v_pose")
# The floors: the device forward and backward are not IEEE fp32, so no gate asks more of them than their own operator tests do.
# A loss: LOSS_TOL.  An output: the network's fraction (kgo.TOL, rpgo.TOL).  Adam's m of one teacher-forced step is 0.1 x this step's
# gradient plus 0.9 x a value both sides share, v the same with g^2 (twice the relative error): the gradients' fractions, once and twice.
FLOORS = {"loss": LOSS_TOL, "probe_depth": kgo.TOL, "probe_pose": rpgo.TOL, "m_depth": kgo.TOL, "v_depth": 2 * kgo.TOL,
          "m_pose": rpgo.TOL, "v_pose": 2 * rpgo.TOL}


def yardsticks(golden, layouts=LAYOUTS):
    """(free, forced): name -> the worst of the fixture's fp32 runs at every step: six frame orders for each of `layouts` (the
    runs of the fixture are layout-major).  An ENVELOPE_GATES figure of the teacher-forced form is the worst of both ways the
    fixture takes it: from the fp64 states and from the fp32 run's own."""
    names = [str(n) for n in golden["distances"]]
    runs = [i for i, (layout, _) in enumerate(fixture_runs()) if layout in layouts]
    assert len(golden["free"]) == len(fixture_runs()) and runs
    free, forced = ({name: golden[which][runs][:, :, i].max(axis=0) for i, name in enumerate(names)} for which in ("free", "forced"))
    for i, name in enumerate(str(n) for n in golden["forced_names"]):
        if name in ENVELOPE_GATES:
            forced[name] = np.maximum(forced[name], golden["forced_own"][runs][:, :, i].max(axis=0))
    return free, forced


def fixture_runs():
    """The fp32 runs of the fixture in its order: (layout, frame order), layout-major."""
    return [(layout, order) for layout in LAYOUTS for order in ORDERS]


def gate_table(golden, metric_floors=None, margin=MARGIN):
    """-> {'forced': name -> bounds, 'free': name -> bounds}: one bound a step (None: not gated at that step), `margin` x the
    fixture's yardstick for that quantity and step (ENVELOPE_GATES: the worst of steps 2 .. 8 for every step after the first), floored (FLOORS; `metric_floors`: steps x 4, relative, from `metric_floor`).
    The free run's loss is gated on the running maximum of its envelope, its depth update at FREE_DEPTH_STEPS, the logged metrics
    from the first validated step on."""
    free, forced = yardsticks(golden)
    steps = len(free["loss"])
    table = {"forced": {}, "free": {}}
    for name in FORCED_GATES:
        per_step = [float(forced[name][t]) for t in range(steps)]
        if name in ENVELOPE_GATES:      # the envelope of the steps after the first
            per_step = per_step[:1] + [max(per_step[1:])] * (steps - 1)
        table["forced"][name] = [max(margin * value, FLOORS.get(name, 0.0)) for value in per_step]
    for name in FREE_GATES:
        bounds = []
        for t in range(steps):
            value = float(np.max(free[name][:t + 1])) if name == "loss" else float(free[name][t])
            floor = FLOORS.get(name, 0.0)
            if name in METRICS and metric_floors is not None:
                floor = float(metric_floors[t][METRICS.index(name)])
            gated = not (name == "depth" and t + 1 not in FREE_DEPTH_STEPS) and not (name in METRICS and t + 1 < VALIDATION_START_STEP)
            bounds.append(max(margin * value, floor) if gated else None)
        table["free"][name] = bounds
    return table


def ratios(measured, bounds):
    """measured: one `distances` dict a step; bounds: name -> one bound a step -> name -> [distance / bound, or None] a step."""
    return {name: [None if b is None else d[name] / b for d, b in zip(measured, per_step)] for name, per_step in bounds.items()}


def first_failure(per_step):
    """The (1-based) first step whose ratio is above 1 (or not a number), with the worst ratio -> (step or None, worst)."""
    finite = [r for r in per_step if r is not None]
    worst = max((float("inf") if r != r else r) for r in finite) if finite else 0.0
    for t, r in enumerate(per_step, 1):
        if r is not None and not r <= 1.0:
            return t, worst
    return None, worst


def forced_against(records, dtype=torch.float64, origin=None):
    """The teacher-forced comparison of a run (`records`, one a step, each with its 'state'): for every step ONE oracle step in
    `dtype` from the run's own state of the step before (`origin` for the first: the initial state), compared with the run's state
    of that step -> (distances a step, exact findings a step: step counts, num_batches_tracked, the learning rates)."""
    previous = initial_state(dtype) if origin is None else origin
    measured, findings = [], []
    for record in records:
        want = next(iterate(dtype, 1, start=previous, with_probes=False))
        measured.append(distances(record, want, cast_state(previous, dtype)))
        found = exact_findings(record["state"], want["state"])
        if record["state"]["lr"] != want["state"]["lr"]:
            found.append(f"learning rates {record['state']['lr']}, expected {want['state']['lr']}")
        findings.append(found)
        previous = record["state"]
    return measured, findings
