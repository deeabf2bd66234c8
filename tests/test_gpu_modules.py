"""-m gpu parity tests of the module surface (CBConv2d, CBPoolMax2d, convert) on MI355X against the
golden sequences recorded from the reference and against the oracle's restatement of the module
state machines (conv2d.py), in both execution modes (sync-free / reference-structured ops)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
from optest import gpu_pkg as pkg      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


def golden_net(d, k):
    net = nn.Sequential(
        nn.Conv2d(3, 4, k, padding=k // 2), nn.ReLU(), nn.MaxPool2d(2, 2),
        nn.Conv2d(4, 6, k, padding=k // 2), nn.ReLU(), nn.MaxPool2d(2, 2),
        nn.Conv2d(6, 8, k, padding=k // 2), nn.ReLU(),
        nn.Conv2d(8, 6, 1), nn.ReLU(),
        nn.Conv2d(6, 4, 1)).eval()
    sd = {n[len("param_"):]: torch.from_numpy(v) for n, v in d.items() if n.startswith("param_")}
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.parametrize("name", ["seq_default", "seq_prop1x1", "seq_nocopy", "seq_k3"])
@pytest.mark.parametrize("sync", [False, True])
def test_golden_sequences(pkg, golden_dir, name, sync):
    """4 frames through a converted scene-labeling-shaped net, as executed by the reference on CPU:
    per-layer change maps bit-exact, per-layer state and final output within 1e-4."""
    d = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    base = golden_net(d, int(d["k"]))
    cb = pkg.convert(base, threshold=float(d["threshold"]))
    assert [n for n, _ in cb.named_children()] == d["childNames"].tolist()
    cbmods = [m for m in cb.modules() if type(m) is pkg.CBConv2d]
    if name == "seq_prop1x1":
        cbmods[2].propChangeIndexes = True       # as sceneLabeling/modelLoader.py:43-44
        cbmods[3].propChangeIndexes = True
    for m in cbmods:
        m.saveChangeMap = True
        m.copyInput = name != "seq_nocopy"
    pkg.setSyncIndexes(cb, sync)
    pkg.clearMemory(cb)
    with torch.no_grad():
        for t in range(4):
            y = cb(torch.from_numpy(d["frame%d" % t]).cuda())
            for li, m in enumerate(cbmods):
                key = "cm%d_l%d" % (t, li)
                if key in d:
                    assert np.array_equal(m.changeMap.cpu().numpy(), d[key]), (t, li)
                np.testing.assert_allclose(m.prevOutput.cpu().numpy(), d["prevOutput%d_l%d" % (t, li)],
                                           rtol=0, atol=FP32_TOL)
            np.testing.assert_allclose(y.cpu().numpy(), d["out%d" % t], rtol=0, atol=FP32_TOL)


def build_oracle_twin(oracle, test_model, pkg):
    """Mirror a (possibly experiment-configured) test model as oracle state machines."""
    layers = []
    for m in test_model.children():
        if type(m) is pkg.CBConv2d:
            layers.append(oracle.OracleCBConv2d(
                m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(), m.threshold,
                withReLU=m.withReLU, feedbackLoop=m.feedbackLoop, propChangeIndexes=m.propChangeIndexes,
                finegrained=m.finegrained, copyInput=m.copyInput))
        elif type(m) is pkg.CBPoolMax2d:
            layers.append(oracle.OracleCBPoolMax2d(ceil_mode=m.ceil_mode,
                                                   propChangeIndexes=m.propChangeIndexes))
        elif type(m) is nn.ReLU:
            layers.append(oracle.OracleReLU())
        elif type(m) is nn.MaxPool2d:
            layers.append(oracle.OracleMaxPool2d(ceil_mode=m.ceil_mode))
        elif type(m) is nn.Conv2d:
            w, b = m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()
            layers.append(type("Dense", (), {
                "forward": lambda self, x, w=w, b=b: oracle.conv2d_dense(x, w, b),
                "clearMemory": lambda self: None})())
        else:
            raise AssertionError(type(m))
    return layers


def _to_np(v):
    if isinstance(v, tuple):
        idx = v[2].tensor() if hasattr(v[2], "tensor") else v[2]
        return (v[0], v[1].cpu().numpy(), idx.cpu().numpy())
    return v.cpu().numpy()


@pytest.mark.parametrize("experiment", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("sync", [False, True])
def test_experiment_presets_vs_oracle(pkg, oracle, experiment, sync):
    """Experiments 1-7 of sceneLabeling/modelLoader.py (incl. feedbackLoop, CBPoolMax2d, fine-grained,
    which have no CPU path in the reference) against the oracle state machines, layer by layer with
    the GPU's own layer inputs (so each layer's mask/index list must match bit-exactly) and end to end."""
    from cbinfer_amd import workloads
    spec = dict(convs=[(3, 8, 7), (8, 12, 7), (12, 20, 7), (20, 12, 1), (12, 5, 1)], pools_after=(0, 1))
    base = workloads.sceneLabelingBaseline(spec, seed=3).cuda()
    test = workloads.configureExperiment(base, pkg.convert(base, threshold=0.03), experiment).cuda()
    pkg.setSyncIndexes(test, sync)
    for m in test.modules():
        if type(m) is pkg.CBConv2d:
            m.saveChangeMap = True
    twin = build_oracle_twin(oracle, test, pkg)
    vid = workloads.SyntheticVideo(H=48, W=64, ratio=0.125, block=8, seed=5)
    pkg.clearMemory(test)
    with torch.no_grad():
        for t, frame in enumerate(vid.frames(4)):
            x = frame
            x_o = frame.cpu().numpy()
            for m, o in zip(test.children(), twin):
                x_in = _to_np(x)
                x = m(x.clone() if isinstance(x, torch.Tensor) else x)
                # teacher-forced oracle layer: same input as the GPU layer saw
                y_o = o.forward(x_in if not isinstance(x_in, tuple) else x_in)
                got = _to_np(x)
                if isinstance(got, tuple):
                    assert np.array_equal(got[2], y_o[2]), (experiment, t, type(m).__name__)
                    got, y_o = got[1], y_o[1]
                if type(m) is pkg.CBConv2d and not m.finegrained and getattr(o, "changeMap", None) is not None \
                        and hasattr(m, "changeMap") and not isinstance(x_in, tuple):
                    assert np.array_equal(m.changeMap.cpu().numpy(), o.changeMap), (experiment, t)
                np.testing.assert_allclose(got, y_o, rtol=0, atol=FP32_TOL)
    # the change-based result tracks the dense model up to the dropped sub-threshold changes
    dense = base(vid.frame)
    assert (x - dense).abs().max().item() < 0.5


def test_first_frame_equals_dense(pkg):
    """+inf initial state => frame 0 recomputes every pixel => equals the dense network (1e-4)."""
    from cbinfer_amd import workloads
    base, test = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05)
    x = torch.rand(1, 3, 320, 480, device="cuda")
    with torch.no_grad():
        y = test(x)
        ref = base(x)
    assert y.shape == ref.shape == (1, 8, 80, 120)
    assert (y - ref).abs().max().item() <= FP32_TOL


def test_state_api(pkg):
    from cbinfer_amd import workloads
    base, test = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05)
    assert all(t.numel() == 0 for t in pkg.getStateTensors(test))
    x = torch.rand(1, 3, 64, 96, device="cuda")
    with torch.no_grad():
        y0 = test(x).clone()
    st = pkg.getStateTensors(test)
    assert len(st) == 3 * 2 + 2 and all(t.numel() > 0 for t in st)   # 3 CBConv2d x2 + 2 pools
    saved = [t.clone() for t in st]                                   # eval03.py:88-95 save/restore
    with torch.no_grad():
        test(torch.rand(1, 3, 64, 96, device="cuda"))
        for t, s in zip(pkg.getStateTensors(test), saved):
            t.copy_(s)
        y1 = test(x)
    assert torch.equal(y0, y1)
    pkg.clearMemory(test)
    assert all(t.numel() == 0 for t in pkg.getStateTensors(test))
    conv = [m for m in test.modules() if type(m) is pkg.CBConv2d][0]
    out = conv(x)
    assert isinstance(out, tuple) and out[0] == 'changeIndexes' and out[1] is conv.prevOutput
    assert 'prevInput' in dict(conv.named_buffers()) and 'prevOutput' in dict(conv.named_buffers())


def test_cpu_tensors_are_rejected(pkg):
    conv = pkg.CBConv2d(nn.Conv2d(3, 4, 3, padding=1), 0.1)
    with pytest.raises(Exception):
        conv(torch.rand(1, 3, 8, 8))


def test_hip_graph_capture(pkg):
    """A whole frame of the converted network is capturable (no sync, no allocation in the library)
    and a replayed graph gives the same result as eager execution."""
    from cbinfer_amd import workloads
    base, eager = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=1)
    _, graphed = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=1)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.1, block=16, seed=3)
    frames = vid.frames(6)
    static_in = frames[0].clone()
    with torch.no_grad():
        graphed(static_in)                       # frame 0 eagerly: allocates state + workspaces
        eager(frames[0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            static_in.copy_(frames[1])
            graphed(static_in)                   # warm-up on the side stream
        torch.cuda.current_stream().wait_stream(s)
        eager(frames[1])
        g = torch.cuda.CUDAGraph()
        static_in.copy_(frames[2])
        with torch.cuda.graph(g):
            static_out = graphed(static_in)
        # capture does not execute: replay frame 2 now, then frames 3..5
        for t in range(2, 6):
            static_in.copy_(frames[t])
            g.replay()
            ref = eager(frames[t])
            assert torch.equal(static_out, ref), t


def test_concurrent_sequences_on_streams(pkg):
    """several sequences in flight on one GPU, one HIP stream and one captured graph each.
    The split-K workspace is keyed by stream, so concurrent replays must not disturb each other: every
    sequence has to reproduce what the same frames give when processed alone, eagerly."""
    from cbinfer_amd import workloads
    S, T = 3, 6
    H, W = 160, 240          # big enough for split-K (few tiles, deep k) in the 64->256 layer
    vids = [workloads.SyntheticVideo(H=H, W=W, ratio=0.1, block=16, seed=11 + q).frames(T) for q in range(S)]
    ref_out = []
    with torch.no_grad():
        for q in range(S):
            _, eager = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=1)
            ref_out.append([eager(f).clone() for f in vids[q]])
        torch.cuda.synchronize()
        runners = []
        for q in range(S):
            _, m = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=1)
            st = torch.cuda.Stream()
            static_in = vids[q][0].clone()
            st.wait_stream(torch.cuda.current_stream())          # weights, frames: made on the default stream
            with torch.cuda.stream(st):
                m(static_in)                                     # frame 0 eagerly (allocations)
                cap = torch.cuda.Stream()
                cap.wait_stream(st)
                with torch.cuda.stream(cap):
                    m(static_in)                                 # warm-up on the capture stream
                st.wait_stream(cap)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=cap):
                    out = m(static_in)
            runners.append((st, static_in, g, out, (cap, m)))   # keep the model (its state tensors) alive
        torch.cuda.synchronize()
        for t in range(1, T):
            for q, (st, static_in, g, out, _) in enumerate(runners):     # all sequences in flight
                with torch.cuda.stream(st):
                    static_in.copy_(vids[q][t])
                    g.replay()
            torch.cuda.synchronize()
            for q, (st, static_in, g, out, _) in enumerate(runners):
                assert (out - ref_out[q][t]).abs().max().item() <= 1e-4, (q, t)


def test_insert_cb_pooling_tracks_dense_and_downsamples_indexes(pkg, oracle):
    """8f-4: automatic change-based pooling.  At threshold 0 the rewritten network must track the dense
    one frame by frame; with downsampleIndexes the pool hands on the list of changed OUTPUT pixels."""
    from cbinfer_amd import workloads
    base = workloads.sceneLabelingBaseline(seed=3).cuda()
    net = pkg.insertCBPooling(pkg.convert(base, threshold=0.0)).cuda()
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.1, block=16, seed=5)
    with torch.no_grad():
        for f in vid.frames(5):
            assert (net(f) - base(f)).abs().max().item() <= FP32_TOL
    conv = pkg.CBConv2d(nn.Conv2d(3, 4, 3, padding=1).cuda(), 0.05)
    conv.propChangeIndexes = True
    pool = pkg.CBPoolMax2d(nn.MaxPool2d(2, 2))
    pool.propChangeIndexes = True
    pool.downsampleIndexes = True
    frames = workloads.SyntheticVideo(H=32, W=48, ratio=0.1, block=8, seed=9).frames(3)
    with torch.no_grad():
        for f in frames:
            tag, out, idx_in = conv(f)
            tag2, pooled, idx_out = pool((tag, out, idx_in))
            assert tag2 == 'changeIndexes'
            want = oracle.poolChangeIndexes(idx_in.tensor().cpu().numpy(), (32, 48), (16, 24))
            assert idx_out.tensor().cpu().numpy().tolist() == want.tolist()
            assert torch.equal(pooled, torch.nn.functional.max_pool2d(out, 2, 2))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("size", [(64, 96, False), (45, 67, False), (45, 67, True)])
def test_pooling_fused_into_detection_is_bit_identical(pkg, dtype, size):
    """fusePoolingIntoDetection: the feedback-mode layer behind a pool computes the pooled values inside
    its change detection (no pool launch, no pooled map).  Outputs and layer states must equal the
    unfused execution bit for bit, for even/odd sizes and floor/ceil pooling."""
    from cbinfer_amd import workloads
    H, W, ceil = size
    def build(fused):
        base = workloads.sceneLabelingBaseline(seed=4, ceil_mode=ceil).to(device='cuda', dtype=dtype)
        net = workloads.configureExperiment(base, pkg.convert(base, threshold=0.05), 6).cuda()
        pkg.fusePoolingIntoDetection(net, enabled=fused)
        return net
    a, b = build(False), build(True)
    assert [m.lazy for m in b.modules() if type(m) is pkg.CBPoolMax2d] == [True, True]
    vid = workloads.SyntheticVideo(H=H, W=W, ratio=0.1, block=1 if (H % 16 or W % 16) else 16, seed=21,
                                   dtype=dtype)
    with torch.no_grad():
        for f in vid.frames(5):
            ya, yb = a(f), b(f)
            # (the dense 1x1 tail of experiment 6 is torch/MIOpen code: its solver choice and split-K reduction
            # are not reproducible from one module instance to the next, so the network outputs are only
            # compared to the last bits; the change-based layers' own states below must be identical)
            if dtype == torch.float32:
                assert torch.allclose(ya, yb, rtol=0, atol=1e-6)
            ca = [m for m in a.modules() if type(m) is pkg.CBConv2d]
            cb = [m for m in b.modules() if type(m) is pkg.CBConv2d]
            for ma, mb in zip(ca, cb):
                assert torch.equal(ma.prevOutput, mb.prevOutput)
                assert torch.equal(ma.prevInput, mb.prevInput)
        # a consumer whose state alone is cleared must see EVERY pixel on its next frame, although the layer
        # in front of it rewrites (and reports in its change mask) only a few: the pooled detection may use the
        # producer's mask only against a state it has compared before
        ca[1].clearMemory()
        cb[1].clearMemory()
        for f in [vid.next(), vid.next()]:
            ya, yb = a(f), b(f)
            for ma, mb in zip(ca, cb):
                assert torch.equal(ma.prevOutput, mb.prevOutput)
                assert torch.equal(ma.prevInput, mb.prevInput)
            assert torch.isfinite(cb[1].prevInput).all()


def test_call_plan_is_dropped_when_its_assumptions_change(pkg, oracle):
    """The per-frame fast path (CBConv2d._run_plan) replays a remembered library call.  Everything it
    depends on is changed here between frames -- threshold, flags, weights (in place and replaced), input
    size, state reset, stream -- and every frame must still equal what a module WITHOUT the fast path
    (CBINFER_NO_FASTPATH) computes."""
    from cbinfer_amd import workloads
    torch.manual_seed(0)

    def build():
        conv = nn.Conv2d(3, 8, 3, padding=1).cuda()
        m = pkg.CBConv2d(conv, 0.05)
        m.feedbackLoop = True
        return m

    fast = build()
    os.environ['CBINFER_NO_FASTPATH'] = '1'
    try:
        slow = build()
        slow.weight.data.copy_(fast.weight.data)
        slow.bias.data.copy_(fast.bias.data)
        vid_a = workloads.SyntheticVideo(H=32, W=64, ratio=0.1, block=8, seed=1).frames(16)
        vid_b = workloads.SyntheticVideo(H=48, W=64, ratio=0.1, block=8, seed=2).frames(4)
        side = torch.cuda.Stream()

        def step(f, both=True):
            os.environ['CBINFER_NO_FASTPATH'] = '0'
            a = fast(f)
            os.environ['CBINFER_NO_FASTPATH'] = '1'
            b = slow(f)
            a = a[1] if isinstance(a, tuple) else a
            b = b[1] if isinstance(b, tuple) else b
            assert torch.equal(a, b)

        with torch.no_grad():
            step(vid_a[0]); step(vid_a[1]); step(vid_a[2])
            assert fast._plan is not None and slow._plan is None
            for m in (fast, slow):
                m.threshold = 0.2                               # threshold
            step(vid_a[3]); step(vid_a[4])
            for m in (fast, slow):
                m.withReLU = True                               # flag
            step(vid_a[5])
            for m in (fast, slow):
                m.weight.data.mul_(1.5)                         # weights in place (version bump)
            step(vid_a[6]); step(vid_a[7])
            for m in (fast, slow):
                m.propChangeIndexes = True                      # tuple output
            step(vid_a[8])
            for m in (fast, slow):
                m.propChangeIndexes = False
            step(vid_b[0]); step(vid_b[1])                      # other input size (state re-allocated)
            step(vid_a[9]); step(vid_a[10])                     # ... and back
            for m in (fast, slow):
                m.clearMemory()                                 # state reset -> 100 % change frame
            step(vid_a[11]); step(vid_a[12])
            torch.cuda.synchronize()
            with torch.cuda.stream(side):                       # another stream (workspace is per stream)
                step(vid_a[13]); step(vid_a[14])
            torch.cuda.synchronize()
            step(vid_a[15])
            step(vid_a[15].transpose(2, 3).contiguous().transpose(2, 3))   # non-contiguous input
    finally:
        os.environ['CBINFER_NO_FASTPATH'] = '0'


def test_half_network(pkg):
    """cg_half path end to end: fp16 network vs the fp32 dense network on the same (fp16-rounded)
    weights, first frame and a changed frame; tolerance 3e-2 absolute on O(1) activations (fp16
    storage of every intermediate)."""
    from cbinfer_amd import workloads
    base, test = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, dtype=torch.float16)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.1, block=16, seed=3, dtype=torch.float16)
    import copy
    ref = copy.deepcopy(base).float()      # base shares its Parameters with the test model
    with torch.no_grad():
        for fr in vid.frames(3):
            y = test(fr)
            assert y.dtype == torch.float16
            r = ref(fr.float())
    assert (y.float() - r).abs().max().item() < 3e-2


@pytest.mark.parametrize("feedback", [False, True])
def test_openpose_half(pkg, feedback):
    """BASELINE config 4 at reduced resolution: the OpenPose T=2 network (36 convs, 185-channel concat)
    converted per sub-model as poseDetection/modelConverter.py:20-24, fp16 (cg_half path), plain and in the
    feedback mode of the reference's pose experiments 10/11 (modelConverter.py:84-86).  Frame 0 must
    equal the dense fp16 network within fp16 accumulation noise; later frames track it up to the dropped
    sub-threshold changes."""
    from cbinfer_amd import workloads
    torch.manual_seed(0)
    base = workloads.OpenPoseModel(T=2, seed=2).cuda().half()
    test = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, seed=2).cuda().half(), threshold=0.01,
                                     feedbackLoop=feedback)
    cbs = [m for m in test.modules() if type(m) is pkg.CBConv2d]
    assert len(cbs) == 36 and all(m.weight.dtype == torch.float16 for m in cbs)
    assert all(m.feedbackLoop == feedback for m in cbs)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.125, block=16, seed=4, dtype=torch.float32)
    frames = [(f * (255.0 / 256.0) - 0.5).half() for f in vid.frames(3)]
    ref32 = workloads.OpenPoseModel(T=2, seed=2).cuda().half().float()
    with torch.no_grad():
        for t, fr in enumerate(frames):
            L, S = test(fr)
            Lr, Sr = ref32(fr.float())
            scale = max(Lr.abs().max().item(), Sr.abs().max().item(), 1e-3)
            err = max((L.float() - Lr).abs().max().item(), (S.float() - Sr).abs().max().item())
            assert L.shape == (1, 38, 8, 12) and S.shape == (1, 19, 8, 12)
            assert err <= (0.02 if t == 0 else 0.1) * scale, (t, err, scale)
    # the two branches of a stage enqueued on two streams: same results, bit for bit
    fork = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, seed=2, concurrentBranches=True).cuda().half(),
                                     threshold=0.01)
    seq = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, seed=2).cuda().half(), threshold=0.01)
    with torch.no_grad():
        for fr in frames:
            (La, Sa), (Lb, Sb) = fork(fr), seq(fr)
            torch.cuda.synchronize()
            assert torch.equal(La, Lb) and torch.equal(Sa, Sb)


def test_pool_without_clone_is_equivalent(pkg):
    """CBPoolMax2d.cloneOutput=False returns the state tensor itself; results are unchanged, also when
    the consumer aliases its input (copyInput=False, no feedback): it then takes the copy itself."""
    from cbinfer_amd import workloads
    for exp, feedback in ((6, True), (6, False)):
        _, a = workloads.sceneLabelingModels(experimentIdx=exp, threshold=0.05, seed=2)
        _, b = workloads.sceneLabelingModels(experimentIdx=exp, threshold=0.05, seed=2)
        for net in (a, b):
            for m in net.modules():
                if type(m) is pkg.CBConv2d:
                    m.feedbackLoop = feedback
                    m.copyInput = False
        for m in b.modules():
            if type(m) is pkg.CBPoolMax2d:
                m.cloneOutput = False
        vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.125, block=16, seed=9)
        with torch.no_grad():
            for f in vid.frames(4):
                ya, yb = a(f.clone()), b(f.clone())
                assert torch.equal(ya, yb)


def test_self_compacting_pipeline_matches_op_sequence(pkg):
    """The default frame pipeline (detection + self-compacting fused kernel, two alternating masks with a
    device-side parity) against the reference-structured op sequence (syncIndexes=True) over a sequence
    with partial changes: identical change lists every frame, states within 1e-5; also across a
    clearMemory() in the middle and with an empty change list (repeated frame)."""
    from cbinfer_amd import workloads
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    _, a = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=5)
    _, b = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.05, seed=5)
    pkg.setSyncIndexes(b, True)
    ca = [m for m in a.modules() if type(m) is pkg.CBConv2d]
    cb_ = [m for m in b.modules() if type(m) is pkg.CBConv2d]
    vid = workloads.SyntheticVideo(H=96, W=160, ratio=0.1, block=16, seed=11)
    frames = vid.frames(7)
    frames.insert(3, frames[2].clone())          # a frame without any change
    with torch.no_grad():
        for t, f in enumerate(frames):
            if t == 5:
                pkg.clearMemory(a)
                pkg.clearMemory(b)
            ya, yb = a(f.clone()), b(f.clone())
            for ma, mb in zip(ca, cb_):
                assert ma._work['selfc'], "self-compacting path not taken"
                ia = ma.lastChangeIndexes().tensor()
                # the op-sequence twin re-derives its list from its own (bit-identical) state
                assert torch.allclose(ma.prevOutput, mb.prevOutput, rtol=0, atol=1e-5), (t,)
                assert torch.allclose(ma.prevInput, mb.prevInput, rtol=0, atol=1e-5), (t,)
                if t == 3:
                    assert ia.numel() == 0
            assert torch.allclose(ya, yb, rtol=0, atol=1e-5)
    # index lists: compare against the detection op on a fresh pair of inputs
    from cbinfer_amd import conv2d_cg as cg
    x0 = torch.rand(1, 3, 96, 160, device="cuda")
    conv = pkg.CBConv2d(torch.nn.Conv2d(3, 16, 7, padding=3).cuda(), 0.05)
    conv.feedbackLoop = True
    with torch.no_grad():
        conv(x0)
        x1 = x0.clone()
        x1[:, :, 10:30, 40:90] += 0.5
        st = conv.prevInput.clone()
        conv(x1)
    expect = cg.changeIndexesExtr(cg.changeDetection(x1, st, (7, 7), 0.05))
    got = conv.lastChangeIndexes().tensor()
    assert torch.equal(got, expect)


def test_fullsize_threshold_zero_tracks_dense(pkg):
    """Size-independent property at BASELINE size (480x320): with threshold 0 every non-zero change is
    detected (strict >), so after any number of frames the change-based network equals the dense network
    on the last frame within the fp32 tolerance -- coarse-grained with feedback loop + change-based
    pooling (experiment 6) -- and a repeated frame leaves every change list empty."""
    from cbinfer_amd import workloads
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    base, test = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.0, seed=3)
    vid = workloads.SyntheticVideo(H=320, W=480, ratio=0.10, block=32, seed=21)
    with torch.no_grad():
        for f in vid.frames(5):
            y = test(f)
        ref = base(vid.frame)
        assert (y - ref).abs().max().item() <= 1e-4
        y2 = test(vid.frame.clone())
        assert torch.equal(y, y2)
        for m in test.modules():
            if type(m) is pkg.CBConv2d:
                assert m.lastChangeIndexes().numel() == 0


def test_eval_harness_and_threshold_tuner(pkg, tmp_path):
    """The reference's measurement protocol (evalTools.inferFramesetBenchmark: last frame timed after
    priming, min of 3) and its greedy threshold tuner with the callback protocol of __init__.py:98-149."""
    from cbinfer_amd import evalTools, workloads
    base, test = workloads.sceneLabelingModels(experimentIdx=4, threshold=0.02, seed=1)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.125, block=16, seed=2)
    frames = [f.cpu() for f in vid.frames(4)]
    t_cb = evalTools.inferFramesetBenchmark(test, frames)
    t_dense = evalTools.inferFramesetBenchmark(base, frames[-1:])
    assert t_cb > 0 and t_dense > 0
    y = evalTools.inferFrameset(test, frames)
    ref = evalTools.inferFrameset(base, frames[-1:])
    assert (y - ref).abs().max().item() < 0.2
    wrapped = torch.nn.Sequential()
    wrapped.add_module('model0', test)
    assert len(evalTools.getCBconvLayers(wrapped)) == 3 and evalTools.getCBpoolLayers(wrapped) == []
    path = evalTools.writeTable([['layer', 'th'], ['0', 0.1]], resultsDir=str(tmp_path))
    assert open(path).read().splitlines() == ['layer,th', '0,0.1']

    class Reader(object):
        def getDataFrames(self, seqName, numFrames):
            return frames[:numFrames], None

    cbs = [m for m in test.modules() if type(m) is pkg.CBConv2d]
    with torch.no_grad():
        target = base(frames[-1].cuda())
    scale = float(target.pow(2).mean())
    pkg.tuneThresholdParameters(Reader(), ['s'], 4, lambda fr: target, lambda fr: fr, base, test,
                                lambda out, tgt: float((out - tgt).pow(2).mean()), cbs,
                                lossToleranceList=1e-4 * scale, initThreshold=1e-3,
                                thresholdIncrFactor=4.0)
    assert all(1e-3 <= m.threshold < 10 for m in cbs), [m.threshold for m in cbs]
    # the tuned network still tracks the dense one: every module stopped before its tolerance was spent
    y2 = evalTools.inferFrameset(test, frames)
    assert float((y2 - ref).pow(2).mean()) <= 4 * 1e-4 * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fuzz_shapes_track_dense(pkg, dtype):
    """Randomised layer shapes (odd sizes, W around the 64-pixel word boundary, K around the 32-row MFMA
    tile, non-square filters, C=1) through the default frame pipeline: with threshold 0 the layer must
    reproduce the dense convolution of the current frame after every frame, and its change list must be
    the dilation of the pixels that actually changed."""
    from cbinfer_amd import conv2d_cg as cg
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    rng = np.random.default_rng(17)
    shapes = [(1, 1, 1, 1, 5, 9), (3, 7, 3, 3, 17, 63), (2, 33, 3, 3, 9, 64), (5, 32, 5, 5, 11, 65),
              (4, 65, 7, 7, 23, 129), (20, 100, 3, 1, 13, 200), (3, 8, 1, 5, 31, 37), (16, 64, 7, 7, 40, 96),
              (7, 3, 3, 3, 64, 64), (1, 16, 7, 7, 8, 300),
              # (round 4: shapes the split-state kernels take -- fp32: 16/32/64 input channels, with and without feedback
              #  loop; fp16: multiples of 64 -- odd maps, non-square filters, K off the tile sizes, shallow and deep)
              (32, 40, 3, 5, 21, 70), (64, 17, 5, 3, 19, 131), (16, 130, 3, 3, 33, 65), (64, 64, 1, 7, 12, 190),
              (128, 70, 3, 3, 27, 66), (192, 33, 1, 3, 15, 129), (64, 200, 5, 5, 18, 64), (256, 64, 3, 1, 9, 77)]
    tol = 1e-4 if dtype == torch.float32 else None
    for (C, K, kH, kW, H, W) in shapes:
        conv = torch.nn.Conv2d(C, K, (kH, kW), padding=(kH // 2, kW // 2)).cuda().to(dtype)
        cbm = pkg.CBConv2d(conv, 0.0)
        cbm.feedbackLoop = bool(rng.integers(0, 2))
        cbm.withReLU = bool(rng.integers(0, 2))
        x = torch.rand(1, C, H, W, device="cuda").to(dtype)
        with torch.no_grad():
            for t in range(4):
                if t:
                    x = x.clone()
                    n = int(rng.integers(1, 4))
                    changed = torch.zeros(H, W, dtype=torch.bool, device="cuda")
                    for _ in range(n):
                        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                        hh, ww = int(rng.integers(1, 6)), int(rng.integers(1, 6))
                        x[:, :, y0:y0 + hh, x0:x0 + ww] += 0.5
                        changed[y0:y0 + hh, x0:x0 + ww] = True
                y = cbm(x.clone())
                ref = conv(x)
                if cbm.withReLU:
                    ref = torch.relu(ref)
                err = (y.float() - ref.float()).abs().max().item()
                bound = tol if tol else 4 * 2.0 ** -10 * max(1.0, ref.float().abs().max().item())
                assert err <= bound, (C, K, kH, kW, H, W, t, err)
                if t:
                    got = cbm.lastChangeIndexes().tensor()
                    expect = cg.changeIndexesExtr(cg.changePropagation(changed.to(torch.int8), (kH, kW)))
                    assert torch.equal(got, expect), (C, K, kH, kW, H, W, t)


# ------------------------------------------------------------------------------------------------
# round 2: fp16 oracle twin, full-size configs 3/4, execution-level fusions, shipped-but-unexercised
# ------------------------------------------------------------------------------------------------
def build_oracle_twin_half(oracle, test_model, pkg):
    layers = []
    for m in test_model.children():
        if type(m) is pkg.CBConv2d:
            layers.append(oracle.OracleCBConv2dHalf(
                m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(), m.threshold,
                withReLU=m.withReLU, feedbackLoop=m.feedbackLoop, propChangeIndexes=m.propChangeIndexes,
                copyInput=m.copyInput))
        elif type(m) is pkg.CBPoolMax2d:
            layers.append(oracle.OracleCBPoolMax2dHalf(ceil_mode=m.ceil_mode,
                                                       propChangeIndexes=m.propChangeIndexes))
        else:
            layers.append(None)        # dense torch module: not part of the cg_half path
    return layers


@pytest.mark.parametrize("experiment", [1, 2, 4, 6])
@pytest.mark.parametrize("sync", [False, True])
def test_half_experiment_presets_vs_oracle(pkg, oracle, experiment, sync):
    """The cg_half MODULE path against its oracle twin (OracleCBConv2dHalf: fp16 operands, exact products
    and sum, one rounding -- cbconv2d_cg_half_backend.cu + conv2d_cg.py:342-349), teacher-forced layer by
    layer like the fp32 preset test: masks and index lists bit-exact, states within 2 fp16 ulp of the
    largest output of the layer (DESIGN.md section 6's fp16 bar)."""
    from cbinfer_amd import workloads
    spec = dict(convs=[(3, 8, 7), (8, 12, 7), (12, 20, 3), (20, 12, 1), (12, 5, 1)], pools_after=(0, 1))
    base = workloads.sceneLabelingBaseline(spec, seed=3).cuda().half()
    test = workloads.configureExperiment(base, pkg.convert(base, threshold=0.03), experiment).cuda()
    pkg.setSyncIndexes(test, sync)
    for m in test.modules():
        if type(m) is pkg.CBConv2d:
            m.saveChangeMap = True
    twin = build_oracle_twin_half(oracle, test, pkg)
    vid = workloads.SyntheticVideo(H=48, W=64, ratio=0.125, block=8, seed=5, dtype=torch.float16)
    checked = 0
    with torch.no_grad():
        for t, frame in enumerate(vid.frames(4)):
            x = frame
            for m, o in zip(test.children(), twin):
                x_in = _to_np(x)
                x = m(x.clone() if isinstance(x, torch.Tensor) else x)
                if o is None:
                    continue
                y_o = o.forward(x_in)
                got = _to_np(x)
                if isinstance(got, tuple):
                    assert np.array_equal(got[2], y_o[2]), (experiment, t, type(m).__name__)
                    got, y_o = got[1], y_o[1]
                if type(m) is pkg.CBConv2d and not isinstance(x_in, tuple):
                    assert np.array_equal(m.changeMap.cpu().numpy(), o.changeMap), (experiment, t)
                assert got.dtype == np.float16
                if type(m) is pkg.CBPoolMax2d:
                    assert np.array_equal(got, y_o)
                else:
                    tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(y_o.astype(np.float32)).max()))
                    np.testing.assert_allclose(got.astype(np.float32), y_o.astype(np.float32), rtol=0, atol=tol)
                checked += 1
    assert checked >= 4 * 3


def test_openpose_fullsize_half_threshold_zero(pkg):
    """BASELINE config 4 at its real size: OpenPose T=2 (poseDetection/openPose/PoseModel.py:34-68,122-137),
    368x654, fp16, all 36 convs converted per sub-model (poseDetection/modelConverter.py:20-24).  The
    368 x 11-word change mask (4048 words) sits just under the self-compacting kernel's limit, Ckk reaches
    9065 (185*49) and the 327-wide map is floor-pooled to 163.  Size-independent property: with threshold 0
    every change is detected, so after several frames the network must equal a fresh evaluation of the
    last frame (same kernels, all-changed) within fp16 accumulation-order noise and track the dense fp16
    torch network within the bar of test_openpose_half's first frame; a repeated frame leaves all 36
    change lists empty and the outputs bit-identical."""
    from cbinfer_amd import workloads
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    H, W = 368, 654
    test = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, seed=2).cuda().half(), threshold=0.0)
    fresh = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, seed=2).cuda().half(), threshold=0.0)
    dense = workloads.OpenPoseModel(T=2, seed=2).cuda().half()
    cbs = [m for m in test.modules() if type(m) is pkg.CBConv2d]
    assert len(cbs) == 36
    gen = torch.Generator(device="cpu").manual_seed(11)
    frame = (torch.rand(1, 3, H, W, generator=gen) * (255.0 / 256.0) - 0.5)
    frames = [frame]
    for t in range(3):              # re-draw 16 blocks of 46 x 109 pixels (~20 % of the frame) per frame
        f = frames[-1].clone()
        for _ in range(16):
            y0 = int(torch.randint(0, H - 46, (1,), generator=gen))
            x0 = int(torch.randint(0, W - 109, (1,), generator=gen))
            f[:, :, y0:y0 + 46, x0:x0 + 109] = torch.rand(1, 3, 46, 109, generator=gen) * (255.0 / 256.0) - 0.5
        frames.append(f)
    frames = [f.cuda().half() for f in frames]
    with torch.no_grad():
        for f in frames:
            L, S = test(f)
        assert L.shape == (1, 38, 46, 81) and S.shape == (1, 19, 46, 81)
        Lf, Sf = fresh(frames[-1])
        Ld, Sd = dense(frames[-1])
        scale = max(Ld.float().abs().max().item(), Sd.float().abs().max().item(), 1e-3)
        err_fresh = max((L.float() - Lf.float()).abs().max().item(), (S.float() - Sf.float()).abs().max().item())
        err_dense = max((L.float() - Ld.float()).abs().max().item(), (S.float() - Sd.float()).abs().max().item())
        print("openpose 368x654 fp16: scale %.4g, vs fresh CB %.3g, vs dense torch %.3g" % (scale, err_fresh, err_dense))
        # measured on MI355X: both 6.1e-5 at scale 0.109, i.e. one fp16 ulp of the largest output; the bar
        # is the fp16 bar of test_fuzz_shapes_track_dense (4 ulp of the largest output)
        assert err_fresh <= 4 * 2.0 ** -10 * scale, (err_fresh, scale)
        assert err_dense <= 4 * 2.0 ** -10 * scale, (err_dense, scale)
        # something must actually have been change-based: frame 3 touched far fewer pixels than frame 0 did
        n1 = cbs[0].lastChangeIndexes().numel()
        assert 0 < n1 < 0.6 * H * W
        L2, S2 = test(frames[-1].clone())
        assert torch.equal(L, L2) and torch.equal(S, S2)
        for m in cbs:
            assert m.lastChangeIndexes().numel() == 0


@pytest.mark.parametrize("form", ["default", "inplace", "atomic"])
def test_fg_fullsize_threshold_zero_tracks_dense(pkg, form):
    """BASELINE config 3 at its real size (experiment 7: fine-grained CBConv2d, 480x320): with threshold 0
    every changed VALUE is propagated, so after several frames the network equals the dense network on the
    last frame within the fp32 bar (1e-4), in every execution form of the fine-grained frame."""
    from cbinfer_amd import workloads
    base, test = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.0, seed=3)
    for m in test.modules():
        if type(m) is pkg.CBConv2d:
            assert m.finegrained
            m.fgInPlace = form == "inplace"
            m.atomicFG = form == "atomic"
    vid = workloads.SyntheticVideo(H=320, W=480, ratio=0.05 if form == "atomic" else 0.10, block=32, seed=21)
    with torch.no_grad():
        for f in vid.frames(4):
            y = test(f.clone())
        ref = base(vid.frame)
        err = (y - ref).abs().max().item()
        assert err <= 1e-4, err
        y2 = test(vid.frame.clone()).clone()
        assert torch.equal(y, y2)


def test_fg_execution_forms_vs_oracle(pkg, oracle):
    """Experiment 7 against the oracle state machine, teacher-forced per layer, in the three execution
    forms (default fused, in-place, reference-structured atomics): outputs <= 1e-4, and the in-place form
    really hands out its own state tensors while the default form hands out fresh ones."""
    from cbinfer_amd import workloads
    spec = dict(convs=[(3, 8, 7), (8, 12, 7), (12, 20, 7), (20, 12, 1), (12, 5, 1)], pools_after=(0, 1))
    for form in ("default", "inplace", "atomic"):
        base = workloads.sceneLabelingBaseline(spec, seed=3).cuda()
        test = workloads.configureExperiment(base, pkg.convert(base, threshold=0.03), 7).cuda()
        cbs = [m for m in test.modules() if type(m) is pkg.CBConv2d]
        for m in cbs:
            m.fgInPlace = form == "inplace"
            m.atomicFG = form == "atomic"
        twin = build_oracle_twin(oracle, test, pkg)
        vid = workloads.SyntheticVideo(H=48, W=64, ratio=0.125, block=8, seed=5)
        outs = []
        with torch.no_grad():
            for t, frame in enumerate(vid.frames(4)):
                x = frame.clone()
                for m, o in zip(test.children(), twin):
                    x_in = x.cpu().numpy()
                    x = m(x)
                    y_o = o.forward(x_in)
                    np.testing.assert_allclose(x.cpu().numpy(), y_o, rtol=0, atol=FP32_TOL)
                    if m is cbs[0]:
                        outs.append(x)
        same = outs[-1].data_ptr() == outs[-2].data_ptr()
        assert same == (form == "inplace")
        if form != "inplace":
            assert cbs[0].prevInput.data_ptr() != cbs[0].prevOutput.data_ptr()


def test_tail1x1_fusion_matches_unfused(pkg, oracle):
    """pycbinfer.fuseTail1x1: experiment 6 with the dense 1x1 tail replaced by one change-based launch.
    Same outputs as the unfused network (<= 1e-4) over a sequence, first frame included; structure:
    the fused module takes the first 1x1 layer's name and shares the parameters."""
    from cbinfer_amd import workloads
    base, plain = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.02, seed=4)
    _, fused = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.02, seed=4)
    names_before = [n for n, _ in fused.named_children()]
    first1x1 = list(fused.children())[-3]
    pkg.fuseTail1x1(fused)
    names = [n for n, _ in fused.named_children()]
    assert names == names_before[:-2]
    tail = list(fused.children())[-1]
    assert type(tail) is pkg.CBTail1x1 and tail.weight1 is first1x1.weight and tail.bias1 is first1x1.bias
    assert list(fused.children())[-2].propChangeIndexes
    pkg.fusePoolingIntoDetection(fused)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.125, block=16, seed=9)
    with torch.no_grad():
        for f in vid.frames(5):
            a, b = plain(f), fused(f)
            assert (a - b).abs().max().item() <= FP32_TOL
        ref = base(vid.frame)
    assert (b - ref).abs().max().item() < 0.5
    assert len(pkg.getStateTensors(fused)) == 2 * 3 + 2 + 1     # 3 convs, 2 pools, the tail
    pkg.clearMemory(fused)
    pkg.clearMemory(plain)         # (both restart from this frame: the feedback-loop state is history-dependent)
    assert tail.prevOutput.numel() == 0
    # graph capture of the fused network (7 launches per frame)
    static_in = vid.frame.clone()
    with torch.no_grad():
        plain(static_in)
        fused(static_in)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fused(static_in)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = fused(static_in)
        nxt = vid.next()
        static_in.copy_(nxt)
        g.replay()
        torch.cuda.synchronize()
        assert (out - plain(nxt)).abs().max().item() <= FP32_TOL


def test_two_graphs_on_the_default_capture_stream_replay_concurrently(pkg):
    """two models captured the natural way (torch.cuda.graph without stream=, i.e. torch's one
    shared capture stream) used to share one split-K workspace keyed by that stream; replayed concurrently
    on different streams they raced.  Each CBConv2d owns its workspace now: concurrent replays must
    reproduce the stand-alone results bit for bit, and capturing allocates nothing."""
    from cbinfer_amd import workloads
    nets, vids, graphs, ins, outs = [], [], [], [], []
    for q in range(2):
        _, test = workloads.sceneLabelingModels(experimentIdx=4, threshold=0.02, seed=q)
        vid = workloads.SyntheticVideo(H=80, W=120, ratio=0.10, block=8, seed=40 + q)
        nets.append(test)
        vids.append(vid.frames(6))
    with torch.no_grad():
        # stand-alone results, eager
        expect = []
        for test, fr in zip(nets, vids):
            for f in fr:
                y = test(f)
            expect.append(y.clone())
            pkg.clearMemory(test)
        for test, fr in zip(nets, vids):
            static = fr[0].clone()
            test(static)
            test(static)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):                  # default (shared) capture stream
                out = test(static)
            graphs.append(g)
            ins.append(static)
            outs.append(out)
        ws = [m._work['conv'].data_ptr() for test in nets for m in test.modules() if type(m) is pkg.CBConv2d]
        assert len(set(ws)) == len(ws)
        streams = [torch.cuda.Stream() for _ in range(2)]
        torch.cuda.synchronize()
        for t in range(1, 6):
            for q in range(2):
                with torch.cuda.stream(streams[q]):
                    ins[q].copy_(vids[q][t])
                    graphs[q].replay()
        torch.cuda.synchronize()
    for q in range(2):
        assert torch.equal(outs[q], expect[q])


def test_propagated_indexes_are_validated(pkg):
    """a change list of another resolution (what CBPoolMax2d hands on by default, like the
    reference, conv2d.py:80-83) or of another dtype must not reach the kernels."""
    from cbinfer_amd._lib import CBinferError
    from cbinfer_amd.conv2d_cg import ChangeIndexes
    conv = pkg.CBConv2d(torch.nn.Conv2d(4, 6, 3, padding=1).cuda(), 0.1)
    x = torch.rand(1, 4, 10, 12, device="cuda")
    with torch.no_grad():
        conv(x)
        with pytest.raises(CBinferError):
            conv(('changeIndexes', x, torch.arange(5, device="cuda")))                 # int64 list
        foreign = ChangeIndexes(torch.zeros(480, dtype=torch.int32, device="cuda"),
                                torch.zeros(1, dtype=torch.int32, device="cuda"), (20, 24))
        with pytest.raises(CBinferError):
            conv(('changeIndexes', x, foreign))
        # an exact int32 list holding an out-of-map entry: the entry is dropped, nothing else is touched
        before = conv.prevOutput.clone()
        x2 = x.clone()
        x2[:, :, 3, 4] += 1.0
        conv.copyInput = True
        lst = torch.tensor([3 * 12 + 4, 10 * 12 + 7], dtype=torch.int32, device="cuda")
        y = conv(('changeIndexes', x2, lst)).clone()
        ref = torch.nn.functional.conv2d(x2, conv.weight, conv.bias, padding=1)
        assert (y[:, :, 3, 4] - ref[:, :, 3, 4]).abs().max().item() <= FP32_TOL
        mask = torch.ones_like(y, dtype=torch.bool)
        mask[:, :, 3, 4] = False
        assert torch.equal(y[mask], before[mask])


def test_compstats_vs_oracle(pkg, oracle):
    """a17: gatherComputationStats (conv2d.py:201-218) against the oracle's numpy restatement, on the first
    frame (state +inf: every value counts as changed) and on a changed frame; totalInputValues is the
    dense op count the 'effective GOp/s' metric divides by."""
    from cbinfer_amd import workloads
    conv = torch.nn.Conv2d(5, 7, (3, 5), padding=(1, 2)).cuda()
    cbm = pkg.CBConv2d(conv, 0.2)
    cbm.gatherComputationStats = True
    rng = np.random.default_rng(2)
    x0 = rng.standard_normal((1, 5, 20, 31)).astype(np.float32)
    x1 = x0.copy()
    x1[0, 1, 4:9, 10:14] += 1.0
    x1[0, 3, 15, 30] -= 0.5
    x1[0, 0, 0, 0] += 0.1          # below the threshold
    with torch.no_grad():
        cbm(torch.from_numpy(x0).cuda())
        first = {k: int(v) for k, v in cbm.compStats.items()}
        assert first == oracle.compStats(x0, np.full_like(x0, np.inf), (7, 5, 3, 5), 0.2)
        assert first["totalInputValues"] == 2 * 5 * 7 * 3 * 5 * 20 * 31
        assert first["numInputChanges"] == first["totalInputValues"]
        cbm(torch.from_numpy(x1).cuda())
        second = {k: int(v) for k, v in cbm.compStats.items()}
    assert second == oracle.compStats(x1, x0, (7, 5, 3, 5), 0.2)
    assert second["numInputChangesPerFeatureMap"] == (20 + 1) * 7 * 3 * 5 * 2
    # the bench's effective-GFLOP/s numerator is the sum of totalInputValues over the converted layers
    _, test = workloads.sceneLabelingModels(experimentIdx=1, threshold=0.05)
    for m in test.modules():
        if type(m) is pkg.CBConv2d:
            m.gatherComputationStats = True
    with torch.no_grad():
        test(torch.rand(1, 3, 32, 48, device="cuda"))
    total = sum(int(m.compStats["totalInputValues"]) for m in test.modules() if type(m) is pkg.CBConv2d)
    assert total == workloads.denseOps(workloads.SCENE_LABELING_SPEC, 32, 48)


def test_power_logger_and_power_measurement(pkg):
    """f3: evalTools.PowerLogger (amdgpu hwmon board power) and inferFramesetPowerMeasurement
    (poseDetection/evalTools.py:54-83: back-and-forth extended frame list under a sampling thread)."""
    from cbinfer_amd import evalTools, workloads
    _, test = workloads.sceneLabelingModels(experimentIdx=4, threshold=0.02, seed=1)
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.125, block=16, seed=2)
    frames = [f.cpu() for f in vid.frames(4)]
    pl = evalTools.inferFramesetPowerMeasurement(test, frames, numFrames=3000, interval=0.01)
    assert len(pl.samples) >= 2
    times = [t for t, _ in pl.samples]
    assert all(b >= a for a, b in zip(times[:-1], times[1:]))
    energy = pl.getTotalEnergy()
    assert energy >= 0.0 and np.isfinite(energy)
    if pl.path is not None and os.access(pl.path, os.R_OK):
        watts = pl.getAveragePower()
        assert np.isfinite(watts) and 5.0 < watts < 2000.0, watts
        assert energy > 0.0
        partial = evalTools.PowerLogger()
        partial.samples = pl.samples[:max(2, len(pl.samples) // 2)]
        assert partial.getTotalEnergy() <= energy + 1e-9          # energy is monotone in time
    else:
        print("no readable amdgpu hwmon power sensor on this box: sampling thread exercised, values NaN")
    pl.recordEvent("done")
    assert pl.events and pl.events[-1][1] == "done"


def test_frame_pipeline_equals_serial_execution(pkg):
    """pycbinfer.FramePipeline: stage 2 of frame t on a side stream while stage 1 of frame t+1 runs.  Every
    frame's output and every layer state after the sequence must be those of the serial execution (the only
    difference allowed: the layer behind the cut detects on a densely pooled tensor instead of pooling inside
    its detection, which is bit-identical by test_pooling_fused_into_detection_is_bit_identical)."""
    from cbinfer_amd import workloads
    def build():
        _, net = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.03, seed=5)
        for m in net.modules():
            if type(m) is pkg.CBPoolMax2d:
                m.cloneOutput = False
        pkg.fuseTail1x1(net)
        pkg.fusePoolingIntoDetection(net)
        return net
    serial, piped = build(), build()
    pipe = pkg.FramePipeline(piped, cut=4)          # conv, pool, conv, pool | conv, tail
    vid = workloads.SyntheticVideo(H=96, W=160, ratio=0.1, block=16, seed=31)
    frames = vid.frames(12)
    outs_p = []
    with torch.no_grad():
        for f in frames:                            # submitted back to back, nothing waited for in between
            y = pipe.submit(f)
            outs_p.append((y, torch.cuda.Event()))
        pipe.wait()
        torch.cuda.synchronize()
        last = y.clone()
        for f in frames:
            ys = serial(f)
        assert torch.equal(last, ys)
    for ms, mp_ in zip([m for m in serial.modules() if type(m) in (pkg.CBConv2d, pkg.CBTail1x1)],
                       [m for m in piped.modules() if type(m) in (pkg.CBConv2d, pkg.CBTail1x1)]):
        assert torch.equal(ms.prevOutput, mp_.prevOutput)
    # used as a plain callable it waits per frame and returns each frame's output
    serial2, piped2 = build(), build()
    pipe2 = pkg.FramePipeline(piped2, cut=4)
    with torch.no_grad():
        for f in frames[:5]:
            a, b = serial2(f).clone(), pipe2(f)
            torch.cuda.synchronize()
            assert torch.equal(a, b)


def test_frame_pipeline_cut_behind_change_indexes(pkg):
    """The cut between a CBConv2d with propChangeIndexes and its CBTail1x1: a ('changeIndexes', tensor, indexes)
    tuple crosses it, so the cloned index buffer and its device-side count are read by the side stream while
    the caller's stream already runs the next frames (advisory, round 2: all three tensors must be tied to the
    side stream).  Frames are submitted back to back; outputs and states must equal the serial execution."""
    from cbinfer_amd import workloads
    def build():
        _, net = workloads.sceneLabelingModels(experimentIdx=6, threshold=0.03, seed=6)
        for m in net.modules():
            if type(m) is pkg.CBPoolMax2d:
                m.cloneOutput = False
        pkg.fuseTail1x1(net)
        pkg.fusePoolingIntoDetection(net)
        return net
    serial, piped = build(), build()
    kids = list(piped.children())
    assert type(kids[4]) is pkg.CBConv2d and kids[4].propChangeIndexes and type(kids[5]) is pkg.CBTail1x1
    pipe = pkg.FramePipeline(piped, cut=5)
    # (the tail would otherwise ride in its producer's second launch -- stage 1 writing a stage-2 module's state while
    #  stage 2 of the frame before still hands that state out: the pipeline keeps the tail's own launch here)
    assert kids[4].__dict__.get('_noTailFold') and kids[4].__dict__['_fusedTail'] is kids[5]
    frames = workloads.SyntheticVideo(H=96, W=160, ratio=0.1, block=16, seed=32).frames(16)
    got, want = [], []
    with torch.no_grad():
        for f in frames:
            y = pipe.submit(f)
            # a private snapshot of this frame's output, taken on the side stream right behind stage 2
            with torch.cuda.stream(pipe.side):
                got.append(y.clone())
            # (allocator pressure on the caller's stream: same-sized temporaries between the frames)
            torch.empty_like(kids[4].prevOutput).fill_(float('nan'))
            torch.empty(96 * 160 // 16, dtype=torch.int32, device='cuda').fill_(-1)
        pipe.wait()
        torch.cuda.synchronize()
        for f in frames:
            want.append(serial(f).clone())
    assert getattr(kids[4].lastChangeIndexes(), 'tailDone', None) is None
    assert getattr([m for m in serial.children()][4].lastChangeIndexes(), 'tailDone', None) is not None
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), t
    for ms, mp_ in zip([m for m in serial.modules() if type(m) in (pkg.CBConv2d, pkg.CBTail1x1)],
                       [m for m in piped.modules() if type(m) in (pkg.CBConv2d, pkg.CBTail1x1)]):
        assert torch.equal(ms.prevOutput, mp_.prevOutput)


def test_producer_mask_shortcut_after_threshold_change(pkg):
    """Advisory (round 2): the pooled detection skips segments the producing layer did not rewrite, which is
    only valid if they compared below the SAME threshold last frame.  Lower a consumer's threshold between
    frames without clearMemory and repeat the frame: pixels whose |pooled - state| lies between the new and
    the old threshold must now be flagged, exactly as in the unfused execution (bit-identical states)."""
    from cbinfer_amd import workloads
    def build(fused):
        base = workloads.sceneLabelingBaseline(seed=4).cuda()
        net = workloads.configureExperiment(base, pkg.convert(base, threshold=0.3), 6).cuda()
        pkg.fusePoolingIntoDetection(net, enabled=fused)
        return net
    a, b = build(False), build(True)
    ca = [m for m in a.modules() if type(m) is pkg.CBConv2d]
    cb = [m for m in b.modules() if type(m) is pkg.CBConv2d]
    vid = workloads.SyntheticVideo(H=64, W=96, ratio=0.25, block=16, seed=23)
    with torch.no_grad():
        frames = vid.frames(4)
        for f in frames:
            a(f), b(f)
        before = cb[1].prevInput.clone()
        for m in (ca[1], cb[1], ca[2], cb[2]):
            m.threshold = 0.01            # lowered; layer 1 keeps 0.3 and so rewrites nothing on a repeated frame
        a(frames[-1]), b(frames[-1])
        assert not torch.equal(before, cb[1].prevInput), "the stimulus must leave sub-old-threshold differences"
        for ma, mb in zip(ca, cb):
            assert torch.equal(ma.prevOutput, mb.prevOutput)
            assert torch.equal(ma.prevInput, mb.prevInput)
        for f in [vid.next(), vid.next()]:     # and the shortcut is back (and still right) afterwards
            a(f), b(f)
            for ma, mb in zip(ca, cb):
                assert torch.equal(ma.prevOutput, mb.prevOutput)
                assert torch.equal(ma.prevInput, mb.prevInput)


@pytest.mark.parametrize("form", ["atomic", "deterministic", "nofused"])
def test_tail_fusion_behind_fine_grained_head_without_touched_list(pkg, form, monkeypatch):
    """Advisory (round 2): fuseTail1x1 switches propChangeIndexes on for a fine-grained head, but only the fused
    frame keeps a list of the output pixels it touched.  The other execution forms (reference-structured atomic
    scatter, deterministic variant, CBINFER_NO_SELFCOMPACT) must still hand CBTail1x1 a tuple -- every pixel --
    and give the unfused network's outputs within 1e-4."""
    from cbinfer_amd import workloads
    if form == "nofused":
        monkeypatch.setenv("CBINFER_NO_SELFCOMPACT", "1")
    base, plain = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.02, seed=4)
    _, fused = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.02, seed=4)
    pkg.fuseTail1x1(fused)
    assert type(list(fused.children())[-1]) is pkg.CBTail1x1
    for net in (plain, fused):
        for m in net.modules():
            if type(m) is pkg.CBConv2d:
                m.atomicFG = form == "atomic"
                m.deterministicFG = form == "deterministic"
    vid = workloads.SyntheticVideo(H=48, W=64, ratio=0.125, block=8, seed=9)
    with torch.no_grad():
        for f in vid.frames(4):
            a, b = plain(f.clone()), fused(f.clone())
            assert (a - b).abs().max().item() <= FP32_TOL


def test_tail_fusion_is_refused_beyond_the_kernels_budget(pkg):
    """fuseTail1x1 checks the one-launch kernel's hidden width AND its LDS budget when the fusion is set up
    (cbinfer_tail1x1_supported), not at the first frame."""
    net = nn.Sequential(nn.Conv2d(8, 512, 3, padding=1), nn.ReLU(), nn.Conv2d(512, 128, 1), nn.ReLU(),
                        nn.Conv2d(128, 96, 1)).eval().cuda()
    cb = pkg.convert(net, threshold=0.1)
    cb = nn.Sequential(*(list(cb.children())[:1] + [net[2], net[3], net[4]]))
    assert not pkg.CBTail1x1.supported(512, 128, 96)
    pkg.fuseTail1x1(cb)
    assert not any(type(m) is pkg.CBTail1x1 for m in cb.modules())
    with torch.no_grad():
        y = cb(torch.rand(1, 8, 16, 24, device="cuda"))
    assert y.shape == (1, 96, 16, 24)
    assert pkg.CBTail1x1.supported(256, 64, 8)


def test_bench_configuration_fullsize_parity(pkg, oracle):
    """THE benchmarked configuration under test at full size (verdict, round 2): bench.build_bench_model() is
    what bench.py times -- experiment 6 (sceneLabeling/modelLoader.py:62-78), fuseTail1x1, pooled detection with
    the producer-mask shortcut, cloneOutput=False, split-state contractions on the DEFAULT arithmetic (bf16 triples,
    f32-equivalent: CBINFER_ARITH=x3) for the 16->64 and 64->256 layers with the tail folded into the second launch,
    row-pair kernel (+ the next layer's pooled detection) for 3->16, threshold 0.05 -- on bench.bench_video():
    480x320, 10 % of the pixels re-drawn per frame in 32x32 blocks, the ping-pong walk with both turn-arounds.
    For every frame (a) each layer is teacher-forced against the oracle twin in the REFERENCE's structure
    (oracle/frame_check.py: change lists bit-exact, feedback states bit-exact, outputs <= 1e-4; reference:
    conv2d.py:178-259, :49-78), and (b) the layer states are bit-identical to the unfused network's."""
    import bench
    from oracle.frame_check import BenchTwin
    from cbinfer_amd import _lib
    base, test = bench.build_bench_model()
    _, plain = bench.build_bench_model(fuse_tail=False, fuse_pool=False, pool_clone=True)
    kids = list(test.children())
    assert [type(m).__name__ for m in kids] == ["CBConv2d", "CBPoolMax2d", "CBConv2d", "CBPoolMax2d", "CBConv2d",
                                                "CBTail1x1"]
    assert all(m.lazy and not m.cloneOutput for m in kids if type(m) is pkg.CBPoolMax2d)
    assert not any(type(m) is pkg.CBTail1x1 or getattr(m, "lazy", False) for m in plain.children())
    convs = [m for m in kids if type(m) is pkg.CBConv2d]
    pconvs = [m for m in plain.children() if type(m) is pkg.CBConv2d]
    assert all(m.threshold == 0.05 and m.feedbackLoop and not m.exactF32 for m in convs + pconvs)
    vid = bench.bench_video(1234)
    assert (vid.H, vid.W, vid.block) == (320, 480, 32) and abs(vid.ratio - 0.10) < 1e-9
    allframes = vid.frames(2 + 4)
    walk = allframes[2:]
    order = [bench.pingpong(i, len(walk)) for i in range(8)]
    assert order == [0, 1, 2, 3, 2, 1, 0, 1]                      # both turn-arounds of the walk
    twin = BenchTwin(pkg, test)
    Ns = []
    with torch.no_grad():
        for t, f in enumerate(allframes[:2] + [walk[i] for i in order]):
            y = twin.step(f, tol=FP32_TOL)
            yp = plain(f)
            for ma, mb in zip(convs, pconvs):
                assert torch.equal(ma.prevOutput, mb.prevOutput), t
                assert torch.equal(ma.prevInput, mb.prevInput), t
            assert (y - yp).abs().max().item() <= FP32_TOL          # (dense torch tail vs the fused launch)
            Ns.append(twin.lastN)
    # the kernels the bench line is about really ran, through their per-layer call plans: the row-segment kernel for
    # 3->16, the split-state kernels (cb_split.hip) for 16->64 and 64->256, the 1x1 tail inside the latter's second
    # launch -- and no layer has fallen back to another arithmetic
    assert convs[0]._plan is not None and not convs[0]._plan.get('split') and convs[0]._plan['rows']
    assert convs[0]._rows_path(torch.float32, *convs[0].prevInput.shape[-2:]) == "rows"
    assert convs[1]._plan is not None and convs[1]._plan['split'] and convs[1]._plan['tail'] is None
    assert convs[2]._plan is not None and convs[2]._plan['split'] and convs[2]._plan['tail'] is kids[-1]
    assert convs[2].lastChangeIndexes().tailDone is kids[-1]
    assert all(m._split_ok(torch.float32, *m.prevInput.shape[-2:]) for m in convs[1:])
    assert not any(m.rangeExceeded() for m in convs)
    assert Ns[0] == [153600, 38400, 9600]                          # first frame: everything
    assert all(n[2] > 3000 and n[0] > 15360 for n in Ns[2:]), Ns   # steady state: 10 % input change, dilated
    # ... and ONLY that: a change mask that is not cleared between frames would keep every pixel "changed" --
    # with identical outputs (round 3 had such a build for an hour; the oracle twin cannot see it, the counts do)
    assert all(n[0] < 0.2 * 153600 and n[1] < 0.35 * 38400 and n[2] < 0.6 * 9600 for n in Ns[2:]), Ns
    # end to end the change-based network stays close to the dense one (sub-threshold changes are dropped)
    assert (y - base(walk[order[-1]])).abs().max().item() < 0.5


def test_bench_inframe_pass_leaves_the_network_intact(pkg):
    """bench.inframe_layer_times issues the library's detection and contraction entry points of every layer by hand (to
    put HIP events around one of them) -- with the arguments the modules themselves would pass: after the pass the
    network's output and every state tensor equal, bit for bit, those of a twin that ran the same frames through the
    modules.  (the hand-made detection call had lost the state's arithmetic bit and wrote f16-pair
    records into a bf16-triple state; nothing noticed.)"""
    import bench
    _, a = bench.build_bench_model()
    _, b = bench.build_bench_model()
    frames = bench.bench_video(77).frames(2 + 6)
    walk = frames[2:]
    with torch.no_grad():
        for f in frames[:2]:
            a(f), b(f)
        for i in range(3):
            a(walk[bench.pingpong(i, len(walk))]), b(walk[bench.pingpong(i, len(walk))])
        got = bench.inframe_layer_times(a, walk, 3, reps=4)
        assert got is not None
        rows, nxt, pair_us = got
        assert nxt > 3 and any("conv_ms" in r for r in rows)
        for i in range(3, nxt):
            yb = b(walk[bench.pingpong(i, len(walk))])
        ya = a(walk[bench.pingpong(nxt, len(walk))])
        yb = b(walk[bench.pingpong(nxt, len(walk))])
        torch.cuda.synchronize()
    assert torch.equal(ya, yb)
    for ta, tb in zip(pkg.getStateTensors(a), pkg.getStateTensors(b)):
        assert torch.equal(ta, tb)
    # the isolated-layer pass brackets the same two entry points through the modules' call plans
    iso = bench.isolated_layers(a, reps=4)
    assert len(iso) == 3 and all(r["conv_us"] > 0 for r in iso)


def test_window_order_fold_in_the_bench_network(pkg):
    """Round 6: the 16 -> 64 layer's contraction in pooling-window order with the 64 -> 256 layer's pooled detection in its
    epilogue (pycbinfer.fuseDetectionIntoProducer(windowOrder=...), cbinfer_split_conv_next), at module level on the bench
    network: forced on, forced off and 'auto' give the same outputs and the same state tensors, bit for bit, frame by
    frame; forced on the form is what runs (the producer's plan holds the consumer's detection, the consumer's frame is its
    contraction alone); 'auto' takes it at the bench's 10 % and declines it on a sequence that changes in most of its
    pixels (the tiles would not fit one round of the grid)."""
    import bench
    import pycbinfer
    nets = {w: bench.build_bench_model(window_order=w)[1] for w in (True, False, "auto")}
    frames = bench.bench_video(91).frames(9)
    with torch.no_grad():
        for t, f in enumerate(frames):
            ys = {w: n(f) for w, n in nets.items()}
            torch.cuda.synchronize()
            assert torch.equal(ys[True], ys[False]) and torch.equal(ys["auto"], ys[False]), t
            for w in (True, "auto"):
                for ta, tb in zip(pkg.getStateTensors(nets[w]), pkg.getStateTensors(nets[False])):
                    assert torch.equal(ta, tb), (w, t)

    def producer(net):
        convs = [m for m in net.modules() if type(m) is pycbinfer.CBConv2d]
        return convs[1], convs[2]
    for w, want in ((True, True), (False, False), ("auto", True)):
        p16, p64 = producer(nets[w])
        plan = p16._plan
        assert plan is not None and plan.get("split") and (plan.get("keep") is not None) == want, w
        if want:      # (the consumer found its detection done: its library call of the last frame was the contraction alone)
            assert p16.lastChangeIndexes().nextDetect == p64._plan["detectToken"]
        # the change list the producer hands out keeps the reference's row-major order whatever order the tiles had
        idx = p16.lastChangeIndexes().tensor().cpu().numpy()
        assert np.all(np.diff(idx) > 0)
    busy = bench.bench_video(92, ratio=0.6, block=16).frames(6)
    _, auto = bench.build_bench_model(window_order="auto")
    with torch.no_grad():
        for f in busy:
            auto(f)
    torch.cuda.synchronize()
    assert producer(auto)[0]._plan is not None and producer(auto)[0]._plan.get("keep") is None


@pytest.mark.parametrize("flip", ["exactF32", "CBINFER_NO_SPLIT"])
@pytest.mark.parametrize("consumer,window_order", [(1, False), (2, True)])
def test_folded_detection_follows_its_consumer_off_the_split_path(pkg, monkeypatch, flip, consumer, window_order):
    """a producer that runs its consumer's pooled change detection in its own launch (the row-pair 3 -> 16
    layer for the 16 -> 64 one; the 16 -> 64 layer in window order for the 64 -> 256 one) must stop doing so in the very
    frame the consumer leaves the split-state kernels -- exactF32 set, or CBINFER_NO_SPLIT=1, between two steady frames.
    Otherwise the producer refreshes the consumer's state and the consumer, on another path, finds nothing changed and keeps
    stale outputs.  Outputs and states equal those of a twin without the fold, frame by frame."""
    import bench
    _, fused = bench.build_bench_model(window_order=window_order)
    _, plain = bench.build_bench_model(fuse_detect=False)
    convs = lambda net: [m for m in net.modules() if type(m) is pkg.CBConv2d]
    frames = bench.bench_video(93).frames(8)
    with torch.no_grad():
        for t, f in enumerate(frames):
            if t == 4:
                assert convs(fused)[consumer - 1]._plan.get("keep") is not None      # (the fold runs up to here)
                if flip == "exactF32":
                    convs(fused)[consumer].exactF32 = convs(plain)[consumer].exactF32 = True
                else:
                    monkeypatch.setenv("CBINFER_NO_SPLIT", "1")
            yf, yp = fused(f), plain(f)
            torch.cuda.synchronize()
            assert torch.equal(yf, yp), t
            for a, b in zip(convs(fused), convs(plain)):
                assert torch.equal(a.prevOutput, b.prevOutput), t
                assert torch.equal(a.prevInput, b.prevInput), t
    assert not convs(fused)[consumer]._split_ok(torch.float32, *convs(fused)[consumer].prevInput.shape[-2:])


@pytest.mark.parametrize("name", ["seq_half", "seq_half_k3"])
@pytest.mark.parametrize("sync", [False, True])
def test_golden_sequences_half(pkg, golden_dir, name, sync):
    """cg_half at module level against the REFERENCE: 4 frames through its convert()-ed net on CPU half tensors
    (tests/golden/gen_golden.py::gen_half; CBConv2d.forward_normal conv2d.py:178-259 over the half backend's ops,
    cbconv2d_cg_half_backend.cu:10-237).  Every CBConv2d is fed the input the reference's own layer saw
    (prevInput after a copyInput frame), so its change map must match bit for bit; its state within HALF_ULPS
    fp16 ulps at the magnitude |output| + |bias| (the fixtures need <= 1: tests/test_oracle_golden.py)."""
    from test_gpu_ops import half_tol
    d = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    k = int(d["k"])
    net = nn.Sequential(
        nn.Conv2d(3, 4, k, padding=k // 2), nn.ReLU(), nn.MaxPool2d(2, 2),
        nn.Conv2d(4, 6, k, padding=k // 2), nn.ReLU(), nn.MaxPool2d(2, 2),
        nn.Conv2d(6, 8, k, padding=k // 2), nn.ReLU(),
        nn.Conv2d(8, 6, 1), nn.ReLU(),
        nn.Conv2d(6, 4, 1)).eval().half()
    net.load_state_dict({n[len("param_"):]: torch.from_numpy(v) for n, v in d.items() if n.startswith("param_")})
    cb = pkg.convert(net.cuda(), threshold=float(d["threshold"]))
    assert [n for n, _ in cb.named_children()] == d["childNames"].tolist()
    cbmods = [m for m in cb.modules() if type(m) is pkg.CBConv2d]
    assert len(cbmods) == 5 and all(m.weight.dtype == torch.float16 for m in cbmods)
    for m in cbmods:
        m.saveChangeMap = True
    pkg.setSyncIndexes(cb, sync)
    pkg.clearMemory(cb)
    with torch.no_grad():
        for t in range(4):
            for li, m in enumerate(cbmods):
                x = torch.from_numpy(d["prevInput%d_l%d" % (t, li)]).cuda()
                out = m(x)
                assert out.dtype == torch.float16
                assert np.array_equal(m.changeMap.cpu().numpy(), d["cm%d_l%d" % (t, li)]), (t, li)
                ref = d["prevOutput%d_l%d" % (t, li)]
                err = np.abs(out.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max()
                tol = half_tol(ref, m.bias.detach().cpu().numpy())
                assert err <= tol, (t, li, err, tol)
        # and the network as a whole on the frames (free-running: later layers see this implementation's own
        # roundings, so a pixel within an ulp of a threshold may be decided differently -- outputs are compared
        # with the looser end-to-end bar of the reference's dense result)
        pkg.clearMemory(cb)
        for t in range(4):
            y = cb(torch.from_numpy(d["frame%d" % t]).cuda())
        ref = d["out3"]
        assert np.abs(y.cpu().numpy().astype(np.float64) - ref.astype(np.float64)).max() <= float(d["threshold"])


def test_tail_folded_into_the_contraction_matches_its_own_launch(pkg, monkeypatch):
    """The fused 1x1 tail evaluated by the 64->256 layer's second launch (cbinfer_split_forward_tail, the default)
    against the same network with the tail in its own launch (CBINFER_NO_TAILFOLD=1): bit-identical network outputs
    and layer states over a walk of frames, through the per-layer call plans, across a change of the tail's weights
    in mid-sequence (the plan must notice) and across clearMemory()."""
    import copy
    import bench
    _, folded = bench.build_bench_model()
    own = copy.deepcopy(folded)
    kids = list(folded.children())
    head = [m for m in kids if type(m) is pkg.CBConv2d][-1]
    tail = kids[-1]
    assert type(tail) is pkg.CBTail1x1 and head.__dict__["_fusedTail"] is tail
    okids = list(own.children())
    assert [m for m in okids if type(m) is pkg.CBConv2d][-1].__dict__["_fusedTail"] is okids[-1]
    frames = bench.bench_video(77).frames(10)
    seen = []

    def run(net, f, fold):
        monkeypatch.setenv("CBINFER_NO_TAILFOLD", "0" if fold else "1")
        with torch.no_grad():
            y = net(f)
        ci = [m for m in net.children() if type(m) is pkg.CBConv2d][-1].lastChangeIndexes()
        seen.append((fold, getattr(ci, "tailDone", None) is not None))
        return y

    for t, f in enumerate(frames):
        if t == 5:
            with torch.no_grad():          # (bumps the version counters: the call plans must be rebuilt)
                tail.weight2.mul_(1.25)
                okids[-1].weight2.mul_(1.25)
        if t == 8:
            pkg.clearMemory(folded)
            pkg.clearMemory(own)
        ya, yb = run(folded, f, True), run(own, f, False)
        assert torch.equal(ya, yb), t
        for ma, mb in zip(folded.children(), own.children()):
            if type(ma) is pkg.CBConv2d:
                assert torch.equal(ma.prevOutput, mb.prevOutput) and torch.equal(ma.prevInput, mb.prevInput), t
    assert all(done == fold for fold, done in seen)      # the folded form really ran, the other really did not
    # a pipeline cut between the layer and its tail, made AFTER frames have run through a folding call plan, takes
    # effect at once -- for as long as the pipeline lives (the switch is the pipeline's, not the net's)
    pipe = pkg.FramePipeline(folded, cut=len(kids) - 1)
    y = run(folded, frames[-1], True)
    assert seen[-1] == (True, False) and torch.equal(y, run(own, frames[-1], False))
    pipe.close()
    y = run(folded, frames[-1], True)
    assert seen[-1] == (True, True) and torch.equal(y, run(own, frames[-1], False))


def test_module_leaves_and_reenters_the_split_path(pkg, oracle):
    """a feedback-mode layer that runs on the split-state kernels leaves them for a few frames
    (saveChangeMap on; the reference-structured op sequence, setSyncIndexes) and comes back.  The other paths refresh
    prevInput through raw pointers, so the pre-split copy of the state must be made again on re-entry, and the two
    mask protocols must not meet in one buffer: every frame against the oracle's state machine (conv2d.py:178-259)
    -- change list bit-exact, refreshed state bit-exact, outputs <= 1e-4 -- and the split-state kernel must really
    have run before and after."""
    rng = np.random.default_rng(41)
    C, K, H, W = 16, 64, 48, 80
    conv = nn.Conv2d(C, K, 7, padding=3).cuda().eval()
    m = pkg.CBConv2d(conv, 0.1)
    m.feedbackLoop, m.withReLU = True, True
    o = oracle.OracleCBConv2d(conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), 0.1,
                              withReLU=True, feedbackLoop=True, propChangeIndexes=True)
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    ran = []
    with torch.no_grad():
        for t in range(14):
            x = x.copy()
            for _ in range(3):
                y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
                x[0, :, y0:y0 + 8, x0:x0 + 8] = rng.standard_normal((C, 8, 8))
            xn = (x + rng.uniform(-0.03, 0.03, x.shape)).astype(np.float32)      # sub-threshold drift everywhere
            m.saveChangeMap = t in (3, 4)
            m.syncIndexes = t in (7, 8, 9)
            m.exactF32 = t == 11
            out = m(torch.from_numpy(xn).cuda())
            ran.append(bool(m.__dict__.get('_ranSplit')) or bool(m._plan and m._plan.get('split')))
            got = o.forward(xn)
            assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), got[2]), t
            assert np.array_equal(m.prevInput.cpu().numpy(), o.prevInput), t
            err = np.abs(out.cpu().numpy() - o.prevOutput).max()
            assert err <= FP32_TOL, (t, err)
            if m.saveChangeMap:
                assert np.array_equal(m.changeMap.cpu().numpy(), o.changeMap), t
    assert ran == [True, True, True, False, False, True, True, False, False, False, True, False, True, True], ran


@pytest.mark.parametrize("arith", ["f16x2", "x3"])
def test_module_range_flag_falls_back(pkg, oracle, monkeypatch, arith):
    """VERDICT round 3, 1(c) at module level: one state value >= 2^20.  f16 pairs (CBINFER_ARITH=f16x2): the frame that
    brings it is already right (the contraction launch computes the layer from prevInput in plain f32 once the detection
    has raised the flag), the module reports it (rangeExceeded), and within a few polls (no sync) it moves the layer to
    the bf16x3 kernels for good.  bf16 triples (the default): f32's range -- nothing trips, the layer stays on the
    split-state kernels.  Every frame against the oracle."""
    monkeypatch.setenv("CBINFER_ARITH", arith)
    rng = np.random.default_rng(43)
    C, K, H, W = 16, 64, 40, 64
    conv = nn.Conv2d(C, K, 7, padding=3).cuda().eval()
    m = pkg.CBConv2d(conv, 0.1)
    m.feedbackLoop = True
    w, b = conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy()
    o = oracle.OracleCBConv2d(w, b, 0.1, feedbackLoop=True, propChangeIndexes=True)
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    with torch.no_grad():
        for t in range(200):
            x = x.copy()
            y0, x0 = rng.integers(0, H - 6), rng.integers(0, W - 6)
            x[0, :, y0:y0 + 6, x0:x0 + 6] = rng.standard_normal((C, 6, 6))
            if t == 3:
                x[0, 5, 7, 9] = 2.0e6
            out = m(torch.from_numpy(x).cuda())
            if t < 8 or t % 16 == 0 or t > 190:
                got = o.forward(x)
                n = got[2]
                assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), n), t
                X = oracle.genXMatrix(o.prevInput, n, (7, 7)).astype(np.float64)
                mag = np.abs(X) @ np.abs(w.reshape(K, -1)).astype(np.float64).T
                err = np.abs(out.cpu().numpy().reshape(K, -1)[:, n].T - o.prevOutput.reshape(K, -1)[:, n].T)
                assert np.all(err <= 64 * 2.0 ** -24 * mag + 1e-6), (t, float(err.max()))
                assert float(np.abs(out.cpu().numpy() - o.prevOutput)[..., :4, 30:].max()) <= FP32_TOL, t
            else:
                o.forward(x)
            if t == 2:
                assert not m.rangeExceeded()
            if t == 3 and arith == "f16x2":
                assert m.rangeExceeded() and not m.__dict__.get('_rangeFallback')
    if arith == "x3":
        assert not m.rangeExceeded() and m._split_ok(torch.float32, H, W) and m._plan.get('split')
        return
    assert m.__dict__.get('_rangeFallback') and m.rangeExceeded()
    assert not m._split_ok(torch.float32, H, W)
    pkg.clearMemory(m)
    assert m._split_ok(torch.float32, H, W) and not m.rangeExceeded()


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("k", [3, 5])
def test_propagated_indexes_into_a_kxk_consumer(pkg, oracle, sync, k):
    """SURVEY 8f-4 remainder.  A CBConv2d fed propagated change indexes skips its own change
    detection for ANY filter size in the reference (conv2d.py:180-190, :220; experiment-1 wiring,
    sceneLabeling/modelLoader.py:41-44, __init__.py:68-77) and recomputes exactly the listed pixels with the state
    update of :234-238.  (a) That behaviour, with a k x k consumer, against the oracle twin layer by layer (lists
    bit-exact, states <= 1e-4), in both execution modes.  (b) The extension dilatePropagatedIndexes: the incoming list
    dilated by the filter support on the device (cbinfer_dilate_change_indexes) == the oracle's changePropagation of
    the producer's map, bit-exact incl. order, and with a threshold of 0 the network then equals the dense one -- which
    the undilated reference behaviour does not."""
    rng = np.random.default_rng(100 + k)
    base = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.ReLU(), nn.Conv2d(8, 8, k, padding=k // 2), nn.ReLU(),
                         nn.Conv2d(8, 4, 1)).cuda().eval()
    H, W = 37, 70

    def make(dilate):
        cb = pkg.convert(base, threshold=0.0 if dilate else 0.05)
        mods = [m for m in cb.children() if type(m) is pkg.CBConv2d]
        assert len(mods) == 3
        mods[0].propChangeIndexes = True          # the k x k layer takes its indexes from the first one ...
        mods[1].propChangeIndexes = True          # ... and hands its own on to the 1x1 layer
        mods[1].dilatePropagatedIndexes = dilate
        pkg.setSyncIndexes(cb, sync)
        return cb, mods

    # (a) reference behaviour against the oracle twin
    cb, mods = make(False)
    twin = build_oracle_twin(oracle, cb, pkg)
    x = rng.uniform(0, 1, (1, 3, H, W)).astype(np.float32)
    with torch.no_grad():
        for t in range(4):
            x = x.copy()
            for _ in range(3):
                y0, x0 = rng.integers(0, H - 5), rng.integers(0, W - 5)
                x[0, :, y0:y0 + 5, x0:x0 + 5] = rng.uniform(0, 1, (3, 5, 5))
            h = torch.from_numpy(x).cuda()
            for m, o in zip(cb.children(), twin):
                h_in = _to_np(h)
                h = m(h)
                y_o = o.forward(h_in)
                got = _to_np(h)
                if isinstance(got, tuple):
                    assert np.array_equal(got[2], y_o[2]), (t, type(m).__name__)
                    got, y_o = got[1], y_o[1]
                np.testing.assert_allclose(got, y_o, rtol=0, atol=FP32_TOL)
            if t > 0:
                assert 0 < mods[1].lastChangeIndexes().numel() < H * W
    # (b) the dilated list, and the network it makes exact
    cb, mods = make(True)
    dense_err, undilated_err = 0.0, 0.0
    cbu, _ = make(False)
    for m in cbu.modules():
        if type(m) is pkg.CBConv2d:
            m.threshold = 0.0
    with torch.no_grad():
        for t in range(4):
            x = x.copy()
            y0, x0 = rng.integers(0, H - 6), rng.integers(0, W - 6)
            x[0, :, y0:y0 + 6, x0:x0 + 6] = rng.uniform(0, 1, (3, 6, 6))
            xin = torch.from_numpy(x).cuda()
            y = cb(xin)
            n_in = mods[0].lastChangeIndexes().tensor().cpu().numpy()
            cm = np.zeros((1, 1, H, W), np.int8)
            cm.reshape(-1)[n_in] = 1
            want = oracle.changeIndexesExtr(oracle.changePropagation(cm.reshape(H, W), (k, k)))
            assert np.array_equal(mods[1].lastChangeIndexes().tensor().cpu().numpy(), want), t
            d = base(xin)
            dense_err = max(dense_err, float((y - d).abs().max()))
            undilated_err = max(undilated_err, float((cbu(xin) - d).abs().max()))
    assert dense_err <= FP32_TOL
    assert undilated_err > 1e-3          # (the reference's behaviour for k > 1: stale outputs around the changed pixels)


@pytest.mark.parametrize("ratio", [0.01, 0.50])
@pytest.mark.parametrize("form", ["default", "inplace"])
def test_fg_fullsize_sweep_ends_track_dense(pkg, form, ratio):
    """BASELINE config 3 at the two ENDS of its sweep: fine-grained CBConv2d + the
    scene-labeling network at 480x320 with 1 % and with 50 % of the pixels re-drawn per frame (16x16 blocks, the
    sweep's generator).  (a) threshold 0: after a walk of frames the network equals the dense network on the last frame
    within 1e-4; (b) the sweep's threshold 0.05: it stays within the sum of what the dropped sub-threshold changes can
    amount to (a loose end-to-end bar, as for the coarse-grained network) and recomputes at most the touched pixels."""
    from cbinfer_amd import workloads
    for th in (0.0, 0.05):
        base, test = workloads.sceneLabelingModels(experimentIdx=7, threshold=th, seed=3)
        cbs = [m for m in test.modules() if type(m) is pkg.CBConv2d]
        for m in cbs:
            assert m.finegrained
            m.fgInPlace = form == "inplace"
        if form == "inplace":
            pkg.fuseTail1x1(test)
        vid = workloads.SyntheticVideo(H=320, W=480, ratio=ratio, block=16, seed=31)
        with torch.no_grad():
            for f in vid.frames(5):
                y = test(f.clone())
            ref = base(vid.frame)
            err = (y - ref).abs().max().item()
            assert err <= (1e-4 if th == 0.0 else 0.5), (th, err)
        # the first layer's touched pixels: the re-drawn blocks dilated by the 7x7 support, nothing like the whole map
        # at 1 %, (nearly) all of it at 50 %
        ci = cbs[0].lastChangeIndexes()
        if ci is not None:
            frac = ci.numel() / float(320 * 480)
            assert (frac < 0.05) if ratio == 0.01 else (frac > 0.5), (ratio, frac)


def _chain_net(pkg, dtype, feedback, seed):
    torch.manual_seed(seed)
    convs = [nn.Conv2d(24, 64, 3, padding=1), nn.Conv2d(64, 64, 3, padding=1), nn.Conv2d(64, 32, 1),
             nn.Conv2d(32, 48, 5, padding=2)]
    net = nn.Sequential(*[pkg.CBConv2d(c.cuda().to(dtype).eval(), 0.05) for c in convs])
    for m in net:
        m.withReLU, m.feedbackLoop = True, feedback
    return net


def _chain_frames(rng, n, C, H, W, dtype):
    """Frames with changed blocks, exact repeats (the first layer finds nothing), sub-threshold drift (it finds
    nothing either) and drift in ONE pixel that the first layer recomputes but whose output stays below the second
    layer's threshold."""
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    frames = []
    for t in range(n):
        kind = ("block", "same", "block", "drift", "same", "same", "block", "tiny")[t % 8]
        x = x.copy()
        if kind == "block":
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            x[0, :, y0:y0 + 8, x0:x0 + 8] = rng.standard_normal((C, 8, 8))
        elif kind == "tiny":
            x[0, 0, rng.integers(0, H), rng.integers(0, W)] += 0.06
        f = x if kind != "drift" else (x + rng.uniform(-0.01, 0.01, x.shape)).astype(np.float32)
        frames.append(torch.from_numpy(f).cuda().to(dtype))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_chained_layers_skip_idle_frames_bit_identically(pkg, dtype, feedback, monkeypatch):
    """Round 4: a CBConv2d fed the output buffer of another one hands the producer's change count to its two launches
    (cbinfer_cbconv2d_forward_after); a zero there ends them at once.  Same network, same frames, with the chain on
    and off (every layer scanning its whole input, as the reference does, conv2d.py:228-233): outputs, states and
    change lists bit-identical in every frame, and the skip must really have been offered on the idle frames."""
    from cbinfer_amd import conv2d as c2
    H, W = 46, 81
    outs = {}
    for name in ("CBINFER_NO_ROWCONV", "CBINFER_NO_BLOCKCONV", "CBINFER_NO_SPLIT"):
        monkeypatch.setenv(name, "1")      # every layer on the list kernels (the chained entry is theirs), fp32 too
    for chain in (True, False):
        monkeypatch.setattr(c2, "_NO_CHAIN", not chain)
        net = _chain_net(pkg, dtype, feedback, 5)
        frames = _chain_frames(np.random.default_rng(7), 24, 24, H, W, dtype)
        rec, offered = [], []
        with torch.no_grad():
            for f in frames:
                y = net(f)
                rec.append([y.clone()] + [m.prevInput.clone() for m in net] +
                           [m.lastChangeIndexes().tensor().clone() for m in net])
                offered.append([m.__dict__.get('_upNow') is not None for m in net])
        outs[chain] = rec
        if chain:
            assert not any(o[0] for o in offered)                  # the first layer has no producer
            assert all(all(o[1:]) for o in offered[3:]), offered   # plans and tags in place from the third frame on
            counts = [[int(t.numel()) for t in r[-4:]] for r in rec]
            assert any(c[0] == 0 and c[1] == 0 for c in counts[3:])         # idle frames: skipped down the chain
            assert any(c[0] > 0 and c[3] > 0 for c in counts[3:])           # and frames that went all the way
        else:
            assert not any(any(o) for o in offered)
    for t, (a, b) in enumerate(zip(outs[True], outs[False])):
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (t, i)


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["list", "hsplit"])
def test_a_skipped_frame_hands_on_an_empty_mask(pkg, kernels, monkeypatch):
    """A chained fp16 layer whose launches end at once -- its producer rewrote nothing -- publishes a change count of
    zero.  The mask it hands on beside that count (propChangeIndexes: a MaskChangeIndexes on the copy of the frame's
    mask) must be empty too: the early exit used to leave the frame before's there, so a module behind the layer that
    reads the mask (CBPointwise2d, CBUpsample2d, ...) recomputed and handed on that frame's pixels on an idle frame.
    Found by tests/test_gpu_chain.py; in every frame the mask holds exactly the listed pixels."""
    if kernels == "list":
        monkeypatch.setenv("CBINFER_NO_SPLIT", "1")
    net = _chain_net(pkg, torch.float16, False, 5)[:2]
    net[1].propChangeIndexes = True
    frames = _chain_frames(np.random.default_rng(7), 8, 24, 46, 81, torch.float16)
    seen = []
    with torch.no_grad():
        for t, f in enumerate(frames):
            tag, y, ix = net(f)
            assert tag == 'changeIndexes' and ix._made and tuple(ix.size) == (46, 81)
            assert bool(net[1].__dict__['_ranSplit']) == (kernels == "hsplit")
            lst = ix.tensor().cpu().numpy()
            words = ix._mask.cpu().numpy().view(np.uint64)
            bits = np.unpackbits(words.view(np.uint8), bitorder='little').reshape(46, -1)[:, :81]
            assert words.size == 46 * 2 and np.array_equal(np.flatnonzero(bits.reshape(-1)), lst), (kernels, t)
            seen.append((net[1].__dict__.get('_upNow') is not None, int(net[0].lastChangeIndexes().numel()), lst.size))
    # (an idle frame in which the skip was offered and taken, behind a frame that listed something)
    assert any(a[2] > 0 and b == (True, 0, 0) for a, b in zip(seen[2:], seen[3:])), seen


@pytest.mark.gpu
def test_chained_layers_do_not_skip_what_they_must_see(pkg, monkeypatch):
    """The premises of the skip, each broken once: (a) somebody writes to the producer's output buffer through torch
    between the layers; (b) the consumer misses one of the producer's frames; (c) the consumer's state is rewritten
    through torch; (d) the threshold of the consumer moves (feedback mode: its state lies within the OLD threshold of
    the input).  Every case against the same calls with the chain switched off."""
    from cbinfer_amd import conv2d as c2
    dtype, H, W = torch.float16, 40, 72
    res = {}
    for chain in (True, False):
        monkeypatch.setattr(c2, "_NO_CHAIN", not chain)
        torch.manual_seed(3)
        p = pkg.CBConv2d(nn.Conv2d(16, 32, 3, padding=1).cuda().half().eval(), 0.05)
        c = pkg.CBConv2d(nn.Conv2d(32, 32, 3, padding=1).cuda().half().eval(), 0.05)
        c.feedbackLoop = True
        rng = np.random.default_rng(11)
        x = torch.from_numpy(rng.standard_normal((1, 16, H, W)).astype(np.float32)).cuda().half()
        x2 = x.clone()
        x2[0, :, 5:13, 9:17] += 1.0
        log = []
        with torch.no_grad():
            for f in (x, x2, x2, x2):                    # warm: plans, tags, two idle frames
                log.append(c(p(f)).clone())
            mid = p(x2)                                  # (a) idle producer frame, then an in-place torch write
            mid[0, :, 20:24, 30:34] += 0.5
            log.append(c(mid).clone())
            log.append(c(p(x2)).clone())
            x3 = x2.clone()
            x3[0, :, 25:30, 40:50] -= 1.0
            p(x3)                                        # (b) a producer frame the consumer never sees ...
            log.append(c(p(x3)).clone())                 # ... then an idle one it is handed
            log.append(c(p(x3)).clone())
            c.prevInput[0, :, 2:4, 2:4] += 0.25          # (c) the consumer's state rewritten through torch
            log.append(c(p(x3)).clone())
            log.append(c(p(x3)).clone())
            c.threshold = 0.001                          # (d) a smaller threshold on an idle frame
            log.append(c(p(x3 + 0.004)).clone())
            log.append(c(p(x3 + 0.004)).clone())
            log.append(c(p(x3 + 0.004)).clone())
        res[chain] = log
    for t, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), t


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 64, 48, 80), (64, 256, 30, 44)])
def test_module_without_feedback_runs_on_the_split_state_kernels(pkg, oracle, shape):
    """Round 4 (missing #3): what convert() makes -- feedbackLoop=False, copyInput=True,
    conv2d.py:234-236 -- on the split-state kernels: the detection writes EVERY value of the frame into prevInput and
    into its pre-split copy (CBINFER_SPLIT_COPY_ALL), so the gather sees this frame's input everywhere, sub-threshold
    drift in the halo of the changed pixels included.  Every frame against the oracle's state machine: change list
    bit-exact, prevInput == the frame bit for bit, outputs <= 1e-4; and the split-state kernel must really have run."""
    rng = np.random.default_rng(61)
    C, K, H, W = shape
    conv = nn.Conv2d(C, K, 7, padding=3).cuda().eval()
    m = pkg.CBConv2d(conv, 0.1)
    m.withReLU = True
    assert not m.feedbackLoop and m.copyInput
    o = oracle.OracleCBConv2d(conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), 0.1,
                              withReLU=True, feedbackLoop=False, propChangeIndexes=True)
    x = rng.standard_normal((1, C, H, W)).astype(np.float32)
    ran = []
    with torch.no_grad():
        for t in range(8):
            x = x.copy()
            if t not in (3, 4):            # (two frames in which nothing exceeds the threshold)
                for _ in range(2):
                    y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
                    x[0, :, y0:y0 + 8, x0:x0 + 8] = rng.standard_normal((C, 8, 8))
            xn = (x + rng.uniform(-0.03, 0.03, x.shape)).astype(np.float32)      # sub-threshold drift everywhere
            out = m(torch.from_numpy(xn).cuda())
            ran.append(bool(m.__dict__.get('_ranSplit')) or bool(m._plan and m._plan.get('split')))
            got = o.forward(xn)
            assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), got[2]), t
            assert np.array_equal(m.prevInput.cpu().numpy(), xn), t
            err = np.abs(out.cpu().numpy() - o.prevOutput).max()
            assert err <= FP32_TOL, (t, err)
    assert ran == [True] * 8, ran


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 64, 48, 80), (64, 256, 30, 44)])
def test_fine_grained_frame_on_the_split_state_kernels(pkg, oracle, shape, monkeypatch):
    """Round 4 (missing #3): CBConv2d.forward_fg (conv2d.py:160-176, cbconv2d_fg_backend.cu:7-66) in
    its in-place form on the split-state kernels (cbinfer_split_forward_fg): the detection writes d = in - prev where
    |d| > th (0 elsewhere) of EVERY value into the pre-split records, the contraction adds W * delta at the mask's
    pixels.  Every frame against the oracle's fine-grained state machine: outputs (with ReLU) <= 1e-4, prevInput ==
    the frame bit for bit, the touched-pixel list == the dilated any-channel mask; the same frames with the split
    path switched off agree to 1e-4 too; and the split-state kernel must really have run."""
    from cbinfer_amd import conv2d_cg
    rng = np.random.default_rng(67)
    C, K, H, W = shape
    conv = nn.Conv2d(C, K, 7, padding=3).cuda().eval()

    def run(split):
        monkeypatch.setenv("CBINFER_NO_SPLIT_FG", "0" if split else "1")
        m = pkg.CBConv2d(conv, 0.1)
        m.withReLU, m.finegrained, m.copyInput, m.fgInPlace, m.propChangeIndexes = True, True, False, True, True
        o = oracle.OracleCBConv2d(conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), 0.1,
                                  withReLU=True, finegrained=True, copyInput=False)
        r = np.random.default_rng(71)
        x = r.standard_normal((1, C, H, W)).astype(np.float32)
        outs, ran = [], []
        with torch.no_grad():
            for t in range(8):
                x = x.copy()
                if t not in (3, 4):
                    for _ in range(2):
                        y0, x0 = r.integers(0, H - 8), r.integers(0, W - 8)
                        x[0, : C // 2, y0:y0 + 8, x0:x0 + 8] = r.standard_normal((C // 2, 8, 8))    # (half the channels)
                xn = (x + r.uniform(-0.03, 0.03, x.shape)).astype(np.float32)      # sub-threshold drift everywhere
                res = m(torch.from_numpy(xn).cuda())
                out = res[1] if isinstance(res, tuple) else res
                ran.append(bool(m._plan and m._plan.get('fgSplit')) or bool(m.__dict__.get('_ranSplit')))
                want = o.forward(xn)
                assert np.array_equal(m.prevInput.cpu().numpy(), xn), t
                err = np.abs(out.cpu().numpy() - want).max()
                assert err <= FP32_TOL, (split, t, err)
                if t > 0:
                    d = np.abs(xn - prev) > np.float32(0.1)
                    mask = conv2d_cg.changePropagation(torch.from_numpy(d.any(1)[0]).cuda(), (7, 7)).cpu().numpy()
                    got = res[2].tensor().cpu().numpy() if hasattr(res[2], 'tensor') else res[2].cpu().numpy()
                    assert np.array_equal(got, np.flatnonzero(mask.reshape(-1)).astype(np.int32)), t
                prev = xn
                outs.append(out.clone())
        return outs, ran

    a, ranA = run(True)
    b, ranB = run(False)
    assert ranA == [False] + [True] * 7 and not any(ranB), (ranA, ranB)
    for t, (u, v) in enumerate(zip(a, b)):
        assert (u - v).abs().max().item() <= FP32_TOL, t


@pytest.mark.gpu
def test_chain_tags_do_not_travel_with_copies(pkg):
    """The tag a CBConv2d leaves on its output buffer names the module and a device word: a deep copy or a pickle of
    a network that has run frames must not drag either along, and the copy must run (and chain) on its own."""
    import copy
    import io
    torch.manual_seed(2)
    net = nn.Sequential(pkg.CBConv2d(nn.Conv2d(32, 64, 3, padding=1).cuda().half().eval(), 0.05),
                        pkg.CBConv2d(nn.Conv2d(64, 64, 3, padding=1).cuda().half().eval(), 0.05))
    x = torch.randn(1, 32, 40, 72, device="cuda").half()
    with torch.no_grad():
        for _ in range(4):
            y = net(x)
        assert net[1].__dict__.get('_upNow') is not None
        twin = copy.deepcopy(net)
        assert getattr(twin[0].prevOutput, '_cbProduced', None) is None
        buf = io.BytesIO()
        torch.save(net, buf)
        buf.seek(0)
        back = torch.load(buf, weights_only=False)
        assert getattr(back[0].prevOutput, '_cbProduced', None) is None
        for other in (twin, back):
            x2 = x.clone()
            x2[0, :, 4:12, 8:16] += 1.0
            for f in (x, x2, x2, x2):
                a, b = net(f), other(f)
                assert torch.equal(a, b)
            assert other[1].__dict__.get('_upNow') is not None


@pytest.mark.gpu
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("shape", [(64, 64, 3, 46, 81), (128, 128, 3, 45, 67), (128, 38, 3, 30, 44), (512, 64, 1, 33, 50),
                                   (128, 128, 7, 30, 44), (192, 160, 3, 24, 40),
                                   # round 5: OpenPose's deep layers at their size -- 7x7 on 185 channels (padded to 192:
                                   # 147 k-stages), 7x7 on 128 (98), 3x3 on 512 (72): the depth in 4, 8 or 16 chunks --
                                   # and a padded shallow one
                                   (185, 128, 7, 46, 81), (128, 128, 7, 46, 81), (512, 512, 3, 46, 81), (100, 64, 3, 31, 45),
                                   # round 6: contractions of one and two k-stages (1x1 on 64 / 128 channels: OpenPose's
                                   # 128->512, 128->128 and 128->38 layers)
                                   (128, 512, 1, 46, 81), (64, 96, 1, 33, 50), (128, 38, 1, 46, 81)])
def test_half_layers_on_the_split_state_machinery(pkg, oracle, shape, feedback, monkeypatch):
    """Round 4: fp16 layers of 64 and more input channels (padded to a multiple of 64, round 5)
    keep a pixel-major f16 copy of their state and contract by LDS-DMA (cbinfer_hsplit_forward; cbconv2d_cg_half_backend.cu:10-88, :146-197).
    Every frame against the oracle's half state machine: change list bit-exact, prevInput bit-exact (the whole frame
    without feedback loop, the changed pixels with it), outputs within 2 fp16 ulp of the layer's largest output
    (DESIGN section 6's fp16 bar); the same frames on rounds 1-2's list kernel agree to the same bar; shallow and deep
    (>= 48 k-stages: k-split + reduce launch) contractions, 64- and 128-row tiles, odd map widths."""
    from cbinfer_amd import _lib
    C, K, k, H, W = shape
    torch.manual_seed(5)
    conv = nn.Conv2d(C, K, k, padding=k // 2).cuda().half().eval()

    def run(hsplit):
        monkeypatch.setenv("CBINFER_NO_HSPLIT", "0" if hsplit else "1")
        m = pkg.CBConv2d(conv, 0.1)
        m.withReLU, m.feedbackLoop = True, feedback
        o = oracle.OracleCBConv2dHalf(conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), 0.1,
                                      withReLU=True, feedbackLoop=feedback, propChangeIndexes=True)
        r = np.random.default_rng(73)
        x = r.standard_normal((1, C, H, W)).astype(np.float16)
        outs, ran = [], []
        with torch.no_grad():
            for t in range(7):
                x = x.copy()
                if t not in (3, 4):
                    for _ in range(2):
                        y0, x0 = r.integers(0, H - 8), r.integers(0, W - 8)
                        x[0, :, y0:y0 + 8, x0:x0 + 8] = r.standard_normal((C, 8, 8)).astype(np.float16)
                xn = (x.astype(np.float32) + r.uniform(-0.03, 0.03, x.shape)).astype(np.float16)
                out = m(torch.from_numpy(xn).cuda())
                ran.append(bool(m._plan and m._plan.get('fn') is _lib.C.cbinfer_hsplit_forward_group))
                got = o.forward(xn)
                assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), got[2]), (hsplit, t)
                assert np.array_equal(m.prevInput.cpu().numpy(), o.prevInput), (hsplit, t)
                ref = o.prevOutput.astype(np.float32)
                tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))
                err = np.abs(out.float().cpu().numpy() - ref).max()
                assert err <= tol, (hsplit, t, err, tol)
                outs.append(out.clone())
        return outs, ran

    a, ranA = run(True)
    b, ranB = run(False)
    assert all(ranA[1:]) and not any(ranB), (ranA, ranB)


@pytest.mark.gpu
@pytest.mark.parametrize("feedback", [False, True])
def test_openpose_fullsize_chain_on_and_off_bit_identical(pkg, feedback, monkeypatch):
    """BASELINE config 4 as the bench runs it (OpenPose T=2, 368x654, fp16, threshold 0.02, random weights: the change
    dies out behind the fifth conv) over 40 frames, with the chained launches (cbinfer_*_after: a layer skips its frame
    on the device when its producer's change count is zero) and with every layer scanning its whole input: the two
    heat-map outputs bit-identical in every frame, eager and replayed from a hipGraph."""
    from cbinfer_amd import conv2d as c2, workloads
    H, W = 368, 654
    vid = workloads.SyntheticVideo(H=H, W=672, ratio=0.10, block=16, seed=3)
    frames = [(f[:, :, :, :W] * (255.0 / 256.0) - 0.5).half().contiguous() for f in vid.frames(40)]
    outs = {}
    for chain in (True, False):
        monkeypatch.setattr(c2, "_NO_CHAIN", not chain)
        torch.manual_seed(0)
        net = workloads.convertOpenPose(workloads.OpenPoseModel(T=2).cuda().half(), threshold=0.02,
                                        feedbackLoop=feedback)
        got = []
        with torch.no_grad():
            for f in frames[:24]:
                y = net(f)
                got.append([t.clone() for t in (y if isinstance(y, (tuple, list)) else [y])])
            static = frames[24].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                y = net(static)
            torch.cuda.current_stream().wait_stream(side)
            got.append([t.clone() for t in (y if isinstance(y, (tuple, list)) else [y])])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                y = net(static)
            for f in frames[25:]:
                static.copy_(f)
                g.replay()
                got.append([t.clone() for t in (y if isinstance(y, (tuple, list)) else [y])])
        torch.cuda.synchronize()
        if chain:
            convs = [m for m in net.modules() if type(m) is pkg.CBConv2d]
            assert sum(1 for m in convs if m.__dict__.get('_upNow') is not None) >= 20      # the chain was offered
        outs[chain] = got
    assert len(outs[True]) == len(outs[False]) == 40
    for t, (a, b) in enumerate(zip(outs[True], outs[False])):
        for u, v in zip(a, b):
            assert torch.equal(u, v), t


@pytest.mark.gpu
@pytest.mark.parametrize("feedback", [False, True])
def test_half_split_state_layer_follows_a_restored_state(pkg, oracle, feedback):
    """eval03.py:88-95 restores layer states from outside.  An fp16 layer on the split-state machinery keeps a
    pixel-major copy of prevInput: after prevInput (and prevOutput) are overwritten through torch the copy must be
    made again -- every following frame against the oracle whose state was set the same way."""
    C, K, H, W = 128, 96, 33, 50
    torch.manual_seed(9)
    conv = nn.Conv2d(C, K, 3, padding=1).cuda().half().eval()
    m = pkg.CBConv2d(conv, 0.1)
    m.withReLU, m.feedbackLoop = True, feedback
    o = oracle.OracleCBConv2dHalf(conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), 0.1,
                                  withReLU=True, feedbackLoop=feedback, propChangeIndexes=True)
    r = np.random.default_rng(79)
    x = r.standard_normal((1, C, H, W)).astype(np.float16)
    saved = None
    with torch.no_grad():
        for t in range(9):
            x = x.copy()
            y0, x0 = r.integers(0, H - 8), r.integers(0, W - 8)
            x[0, :, y0:y0 + 8, x0:x0 + 8] = r.standard_normal((C, 8, 8)).astype(np.float16)
            if t == 6:      # back to the state after frame 2
                m.prevInput.copy_(torch.from_numpy(saved[0]).cuda())
                m.prevOutput.copy_(torch.from_numpy(saved[1]).cuda())
                o.prevInput, o.prevOutput = saved[0].copy(), saved[1].copy()
            out = m(torch.from_numpy(x).cuda())
            got = o.forward(x)
            assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), got[2]), t
            assert np.array_equal(m.prevInput.cpu().numpy(), o.prevInput), t
            ref = o.prevOutput.astype(np.float32)
            tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(ref).max()))
            assert np.abs(out.float().cpu().numpy() - ref).max() <= tol, t
            if t == 2:
                saved = (m.prevInput.cpu().numpy().copy(), m.prevOutput.cpu().numpy().copy())
    assert m._plan is not None and m._plan.get('stateVersion') is not None      # (the split-state path, with its plan)


@pytest.mark.gpu
def test_fg_with_change_based_pools_fullsize_threshold_zero(pkg):
    """BASELINE.json configs[2] word for word -- fine-grained CBConv2d + CBPoolMax2d -- at 480x320: the fine-grained
    head hands the pixels it touched to the change-based pool (an extension: the reference's forward_fg hands on no
    indexes, conv2d.py:160-176), which recomputes the windows that hold one.  With threshold 0 the network must track
    the dense one."""
    from cbinfer_amd import workloads
    base, fg = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.0)
    for m in fg.modules():
        if type(m) is pkg.CBConv2d:
            m.fgInPlace = True
    pkg.insertCBPooling(fg, cloneOutput=False)
    pkg.fuseTail1x1(fg)
    assert sum(1 for m in fg.modules() if type(m) is pkg.CBPoolMax2d) == 2
    vid = workloads.SyntheticVideo(H=320, W=480, ratio=0.1, block=16, seed=5)
    frames = vid.frames(10)
    worst = 0.0
    with torch.no_grad():
        for f in frames:
            worst = max(worst, (fg(f) - base(f)).abs().max().item())
    assert worst <= FP32_TOL, worst
    # ... and with the pools folded into the fine-grained detections (cbinfer_split_forward_fg, pooled form): no pool
    # launch, the pooled maps only in the layers' states
    _, fz = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.0)
    for m in fz.modules():
        if type(m) is pkg.CBConv2d:
            m.fgInPlace = True
    pkg.insertCBPooling(fz, cloneOutput=False)
    pkg.fuseTail1x1(fz)
    pkg.fusePoolingIntoDetection(fz)
    pools = [m for m in fz.modules() if type(m) is pkg.CBPoolMax2d]
    assert len(pools) == 2 and all(p.lazy for p in pools)
    worst = 0.0
    with torch.no_grad():
        for f in frames:
            worst = max(worst, (fz(f) - base(f)).abs().max().item())
    assert worst <= FP32_TOL, worst
    convs = [m for m in fz.modules() if type(m) is pkg.CBConv2d]
    assert all(m._plan is not None and m._plan.get('fgSplit') and m._plan['pooled'] for m in convs[1:])
    assert all(p.outputState.numel() == 0 for p in pools)      # (the pooled maps were never materialised)


@pytest.mark.gpu
def test_pools_fold_into_the_detection_of_layers_without_feedback(pkg):
    """What convert() makes (experiment 2: feedbackLoop=False, copyInput=True) with its pools change-based
    (insertCBPooling): fusePoolingIntoDetection folds them into the copy-all detections of the split-state layers
    (round 4) -- an execution-level fusion: the same frames with and without it give bit-identical outputs, layer
    states and change lists; with threshold 0 the network tracks the dense one; and the pooled maps are never
    materialised."""
    from cbinfer_amd import workloads
    vid = workloads.SyntheticVideo(H=320, W=480, ratio=0.1, block=16, seed=9)
    frames = vid.frames(9)
    for th in (0.05, 0.0):
        nets = []
        for fuse in (True, False):
            base, net = workloads.sceneLabelingModels(experimentIdx=2, threshold=th)
            pkg.insertCBPooling(net, cloneOutput=False)
            pkg.fusePoolingIntoDetection(net, enabled=fuse)
            nets.append(net)
        pools = [m for m in nets[0].modules() if type(m) is pkg.CBPoolMax2d]
        assert len(pools) == 2 and all(p.lazy for p in pools)
        with torch.no_grad():
            for t, f in enumerate(frames):
                a, b = nets[0](f), nets[1](f)
                assert torch.equal(a, b), (th, t)
                for ma, mb in zip([m for m in nets[0].modules() if type(m) is pkg.CBConv2d],
                                  [m for m in nets[1].modules() if type(m) is pkg.CBConv2d]):
                    assert torch.equal(ma.prevInput, mb.prevInput), (th, t)
                    assert torch.equal(ma.lastChangeIndexes().tensor(), mb.lastChangeIndexes().tensor()), (th, t)
                if th == 0.0:
                    assert (a - base(f)).abs().max().item() <= FP32_TOL, t
        convs = [m for m in nets[0].modules() if type(m) is pkg.CBConv2d]
        assert all(m._plan is not None and m._plan.get('split') and m._plan['pooled'] for m in convs[1:3])
        assert all(p.outputState.numel() == 0 for p in pools)


@pytest.mark.gpu
@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("size", [(46, 82), (45, 67)])
def test_pools_fold_into_the_fp16_split_state_detection(pkg, feedback, size):
    """An fp16 chain conv -> CBPoolMax2d -> conv -> CBPoolMax2d -> conv (64/128/256 channels: the split-state fp16
    kernels) with the pools folded into the consumers' detections (cbinfer_hsplit_forward, pooled form; the producer's
    mask tells it which segments to look at) and with pool launches of their own: outputs, layer states and change
    lists bit-identical in every frame; even and odd maps (floor pooling of an odd size)."""
    H, W = size
    nets = []
    for fuse in (True, False):
        torch.manual_seed(21)
        convs = [nn.Conv2d(64, 64, 3, padding=1), nn.Conv2d(64, 128, 3, padding=1), nn.Conv2d(128, 256, 3, padding=1)]
        mods = []
        for i, c in enumerate(convs):
            m = pkg.CBConv2d(c.cuda().half().eval(), 0.05)
            m.withReLU, m.feedbackLoop = True, feedback
            mods.append(m)
            if i < 2:
                mods.append(nn.MaxPool2d(2, 2))
        net = nn.Sequential(*mods)
        pkg.insertCBPooling(net, cloneOutput=False)
        pkg.fusePoolingIntoDetection(net, enabled=fuse)
        nets.append(net)
    pools = [m for m in nets[0] if type(m) is pkg.CBPoolMax2d]
    assert len(pools) == 2 and all(p.lazy for p in pools)
    rng = np.random.default_rng(23)
    x = rng.standard_normal((1, 64, H, W)).astype(np.float16)
    with torch.no_grad():
        for t in range(8):
            x = x.copy()
            if t not in (4,):
                y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
                x[0, :, y0:y0 + 8, x0:x0 + 8] = rng.standard_normal((64, 8, 8)).astype(np.float16)
            f = torch.from_numpy(x).cuda()
            a, b = nets[0](f), nets[1](f)
            assert torch.equal(a, b), t
            for ma, mb in zip([m for m in nets[0] if type(m) is pkg.CBConv2d],
                              [m for m in nets[1] if type(m) is pkg.CBConv2d]):
                assert torch.equal(ma.prevInput, mb.prevInput), t
                assert torch.equal(ma.lastChangeIndexes().tensor(), mb.lastChangeIndexes().tensor()), t
    convs0 = [m for m in nets[0] if type(m) is pkg.CBConv2d]
    from cbinfer_amd import _lib
    assert all(m._plan is not None and m._plan['fn'] is _lib.C.cbinfer_hsplit_forward_group and m._plan['pooled']
               for m in convs0[1:])
    assert all(p.outputState.numel() == 0 for p in pools)


@pytest.mark.gpu
def test_openpose_live_network_fullsize(pkg, oracle):
    """BASELINE config 4 on the LIVE network the bench measures (round 5: workloads.OpenPoseModel(init='kaiming'),
    per-layer thresholds from workloads.calibrateChangeRatio), full size 368x654, fp16.
    (1) threshold-0 property: with every threshold 0 the change-based network recomputes exactly the pixels whose
        input differs (strict >, cbconv2d_cg_half_backend.cu:27-28), so its two heat-map outputs track the dense
        network's on the same weights -- every layer busy, the 185-channel layers padded to 192, the deep contractions
        split 4..16 ways -- within the fp16 bar of 36 chained layers;
    (2) at the calibrated thresholds every layer recomputes (no dead tail as on nn.Conv2d's default initialisation), and
        ALL 36 layers (round 6; round 5 forced three) are TEACHER-FORCED against the oracle's half state machine on the
        inputs the running network hands them -- with the consumers' change detection running inside the producers'
        launches (29 of the 36 detections): change lists bit-exact, prevInput bit-exact, outputs within 2 fp16 ulp of the
        layer's largest output."""
    from cbinfer_amd import workloads, _lib
    H, W = 368, 654
    vid = workloads.SyntheticVideo(H=H, W=672, ratio=0.10, block=16, seed=11)

    def prep(f):
        return (f[:, :, :, :W] * (255.0 / 256.0) - 0.5).half().contiguous()

    def live():
        return workloads.OpenPoseModel(T=2, init='kaiming').cuda().half()
    dense = live()
    # (1) threshold 0
    net0 = workloads.convertOpenPose(live(), threshold=0.0)
    with torch.no_grad():
        for t in range(4):
            f = prep(vid.next())
            a, b = net0(f), dense(f)
            for u, v in zip(a, b):
                ref = v.float()
                tol = 0.03 * float(ref.abs().max())
                err = float((u.float() - ref).abs().max())
                assert err <= tol, (t, err, tol)
    convs0 = [m for m in net0.modules() if type(m) is pkg.CBConv2d]
    assert all(m.lastChangeIndexes().numel() > 0 for m in convs0)
    paths = [m._plan['fn'] for m in convs0 if m._plan is not None and m._plan.get('fn') is not None]
    assert sum(1 for p in paths if p is _lib.C.cbinfer_hsplit_forward_group) == 35      # (all but the 3-channel layer)
    del net0
    # (2) calibrated thresholds, EVERY layer teacher-forced, in the execution form the bench measures: the consumers'
    #     detection inside the producers' launches (workloads.fuseOpenPoseDetections)
    net = workloads.fuseOpenPoseDetections(workloads.convertOpenPose(live(), threshold=0.02))
    ths = workloads.calibrateChangeRatio(net, lambda: prep(vid.next()), target=0.10, pairs=3, settle=6, finalSettle=12)
    convs = [m for m in net.modules() if type(m) is pkg.CBConv2d]
    assert len(ths) == 36 and all(th >= 0 for th in ths)
    twins, captured = {}, {}
    for m in convs:
        twins[m] = oracle.OracleCBConv2dHalf(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(),
                                             float(m.threshold), withReLU=bool(m.withReLU), feedbackLoop=False,
                                             propChangeIndexes=True)
        # the twin starts from the layer's present state
        twins[m].prevInput = m.prevInput.cpu().numpy().copy()
        twins[m].prevOutput = m.prevOutput.cpu().numpy().copy()
        m.register_forward_pre_hook(lambda mod, inp: captured.__setitem__(mod, inp[0].detach().cpu().numpy().copy()))
    counts = np.zeros(len(convs))
    folded = np.zeros(len(convs), dtype=int)
    frames_checked = 3
    with torch.no_grad():
        for t in range(frames_checked):
            net(prep(vid.next()))
            torch.cuda.synchronize()
            counts += [m.lastChangeIndexes().numel() for m in convs]
            for i, m in enumerate(convs):
                o = twins[m]
                got = o.forward(captured[m])
                hs = m._work.get('hsplit')
                if hs is not None:
                    assert m._plan is not None and m._plan.get('fn') is _lib.C.cbinfer_hsplit_forward_group
                    folded[i] += int(hs['layer'][0].detect == 0)
                assert np.array_equal(m.lastChangeIndexes().tensor().cpu().numpy(), got[2]), (t, i, m.weight.shape)
                assert np.array_equal(m.prevInput.cpu().numpy(), o.prevInput), (t, i, m.weight.shape)
                ref = o.prevOutput.astype(np.float32)
                tol = 2 * 2.0 ** -10 * max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))
                err = np.abs(m.prevOutput.float().cpu().numpy() - ref).max()
                assert err <= tol, (t, i, m.weight.shape, err, tol)
    ratios = counts / float(frames_checked) / np.array([m.prevInput.size(-1) * m.prevInput.size(-2) for m in convs],
                                                       dtype=np.float64)
    assert ratios.min() > 0.01 and 0.04 < ratios.mean() < 0.25, ratios      # every layer alive, ~10 % on average
    # all layers but the 3-channel one on the split-state machinery (the 1x1 layers too, round 6); the detection of every
    # layer directly behind another one -- 7 in the feature extractor, 2 x 5 in stage 1 (the heads behind the extractor's
    # last layer), 2 x 6 in stage 2 -- ran in its producer's launch in every checked frame
    assert sum(1 for m in convs if m._work.get('hsplit') is not None) == 35
    assert int((folded == frames_checked).sum()) == 29, folded


@pytest.mark.gpu
@pytest.mark.parametrize("pools", [False, True])
def test_fine_grained_tail_rides_in_the_second_launch(pkg, monkeypatch, pools):
    """Round 5: the fine-grained experiment 7 network in its in-place form with the fused 1x1 tail
    evaluated by the 64->256 contraction's second launch (cbinfer_split_forward_fg_tail: that launch adds the partial
    tiles' sum to prevOutput, keeps the relu'd copy and runs the tail on it) against the same network with the tail's
    own launch (CBINFER_NO_TAILFOLD=1): network outputs, layer outputs and relu'd copies bit-identical over a walk with
    idle frames, at 480x320, with nn.MaxPool2d and with change-based pools folded into the fine-grained detections; and
    the fold really runs."""
    from cbinfer_amd import workloads, _lib

    def build(fold):
        monkeypatch.setenv("CBINFER_NO_TAILFOLD", "0" if fold else "1")
        _, net = workloads.sceneLabelingModels(experimentIdx=7, threshold=0.05)
        for m in net.modules():
            if type(m) is pkg.CBConv2d:
                m.fgInPlace = True
        if pools:
            pkg.insertCBPooling(net, cloneOutput=False)
        pkg.fuseTail1x1(net)
        if pools:
            pkg.fusePoolingIntoDetection(net)
        return net
    vid = workloads.SyntheticVideo(H=320, W=480, ratio=0.10, block=16, seed=5)
    frames = vid.frames(7)
    frames = frames[:3] + [frames[2], frames[2]] + frames[3:]        # (two idle frames)
    outs = {}
    for fold in (True, False):
        net = build(fold)      # (the switch is read when a frame is dispatched: keep it set while this network runs)
        got = []
        with torch.no_grad():
            for f in frames:
                y = net(f)
                head = [m for m in net.children() if type(m) is pkg.CBConv2d][-1]
                got.append((y.clone(), head.prevOutput.clone()))
        if fold:
            assert head._plan is not None and head._plan.get('fn') is _lib.C.cbinfer_split_forward_fg_tail
        else:
            assert head._plan is None or head._plan.get('fn') is not _lib.C.cbinfer_split_forward_fg_tail
        outs[fold] = got
    for t, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert torch.equal(a[0], b[0]), t
        assert torch.equal(a[1], b[1]), t


@pytest.mark.gpu
def test_chained_fp16_layers_skip_what_their_producer_left_alone(pkg, monkeypatch):
    """Round 5: an fp16 split-state layer that is handed another change-based layer's output buffer (a chain) also
    gets that layer's change mask of the frame, and its detection skips the 64-pixel segments the producer did not
    rewrite (cbh_detect_kernel, non-pooled producer-mask shortcut).  The live OpenPose network at full size with
    calibrated thresholds, 12 frames: the two heat-map outputs, every layer's prevInput / prevOutput and change list
    bit-identical with the shortcut on and off (CBINFER_NO_CHAINMASK=1) -- and the shortcut really is offered."""
    from cbinfer_amd import workloads
    H, W = 368, 654

    def prep(f):
        return (f[:, :, :, :W] * (255.0 / 256.0) - 0.5).half().contiguous()
    vid = workloads.SyntheticVideo(H=H, W=672, ratio=0.10, block=16, seed=21)
    net = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, init='kaiming').cuda().half(), threshold=0.02)
    ths = workloads.calibrateChangeRatio(net, lambda: prep(vid.next()), target=0.10, pairs=2, settle=4, finalSettle=4)
    frames = [prep(vid.next()) for _ in range(12)]
    frames[5] = frames[4]                      # (an exact repeat: every count is zero, the chain skips whole layers)
    runs = {}
    for off in ("0", "1"):
        monkeypatch.setenv("CBINFER_NO_CHAINMASK", off)
        m = workloads.convertOpenPose(workloads.OpenPoseModel(T=2, init='kaiming').cuda().half(), threshold=0.02)
        convs = [c for c in m.modules() if type(c) is pkg.CBConv2d]
        for c, th in zip(convs, ths):
            c.threshold = th
        got, offered = [], 0
        with torch.no_grad():
            for f in frames:
                y = m(f)
                offered += sum(1 for c in convs if c._chain_mask(c.prevInput.size(-2), c.prevInput.size(-1)) is not None)
                got.append(([t.clone() for t in y], [c.prevInput.clone() for c in convs],
                            [c.prevOutput.clone() for c in convs],
                            [c.lastChangeIndexes().tensor().clone() for c in convs]))
        runs[off] = (got, offered)
    assert runs["0"][1] >= 15 * 8 and runs["1"][1] == 0, (runs["0"][1], runs["1"][1])
    for t, (a, b) in enumerate(zip(runs["0"][0], runs["1"][0])):
        for part in range(4):
            for u, v in zip(a[part], b[part]):
                assert torch.equal(u, v), (t, part)


def test_first_layer_detects_in_its_own_launch(pkg):
    """Round 6: the 3 -> 16 layer's change detection inside its row-pair launch, its state refresh carried by the
    16 -> 64 layer's contraction -- in window order and in pixel order -- or, where nothing carries it, issued as a launch of
    its own: against the network with the detection launch (CBINFER_NO_PAIRDET=1), outputs and every state tensor bit for
    bit, frame by frame; the library calls of a steady-state frame are the three the form promises."""
    import bench
    import pycbinfer
    from cbinfer_amd import _lib
    frames = bench.bench_video(93).frames(9)
    os.environ["CBINFER_NO_PAIRDET"] = "1"
    try:
        ref = bench.build_bench_model(window_order=False)[1]
        want = []
        with torch.no_grad():
            for f in frames:
                want.append((ref(f).clone(), [t.clone() for t in pkg.getStateTensors(ref)]))
    finally:
        os.environ.pop("CBINFER_NO_PAIRDET")
    for wo, calls_want in ((True, ["cbinfer_conv_rowpairs_detect", "cbinfer_split_conv_next_refresh", "cbinfer_split_conv_tail"]),
                           (False, ["cbinfer_conv_rowpairs_detect", "cbinfer_split_conv_refresh", "cbinfer_cbconv2d_forward" ])):
        net = bench.build_bench_model(window_order=wo)[1]
        with torch.no_grad():
            for t, f in enumerate(frames):
                rec = []
                _lib._RECORDING[0] = rec
                try:
                    y = net(f)
                finally:
                    _lib._RECORDING[0] = None
                torch.cuda.synchronize()
                assert torch.equal(y, want[t][0]), (wo, t)
                for a, b in zip(pkg.getStateTensors(net), want[t][1]):
                    assert torch.equal(a, b), (wo, t)
        names = [fn.__name__ for fn, _ in rec]
        assert names[0] == calls_want[0] and names[1] == calls_want[1], (wo, names)
