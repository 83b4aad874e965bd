"""GPU: training on cached CLIP features.  tri_dropout_tick / tri_dropout_apply (csrc/dropout.hip) against the torch restatement
(ops.dropout_apply on host tensors, itself pinned to the numpy oracle in tests/test_clip_features_cpu.py) bit for bit and inside guard
bands; the tick's semantics eagerly and under HIP-graph replay; CLIPImageEncoder against tests/golden/clip_img.npz (the reference's
class: eval mode in fp32, train mode in float64 with the real counter mask); CLIPTextEncoder(dropout="counter") against a float64
restatement; four Adam steps of Bi(CLIPImageEncoder, CLIPTextEncoder) against a float64 CPU loop; and train.main / test.main end to
end on a tiny packed tree.

Bounds.  Eval parity: z within 2e-4 and gradients through test_gpu_modules._check_grads with GRAD_RTOL, as test_clip_text_matches_reference
and its siblings apply to the same-shaped head.  Train parity: z within 2e-5, parameter gradients within atol 3e-5 / rtol 2e-4, the
bounds of test_clip_text_train_mode_dropout_with_an_injected_mask at the same B = 8 - here with the real mask.  Training steps: the
step-0 loss within LOSS_TOL = 1e-3, later steps within 1e-2, as test_training_steps_match_reference."""
import numpy as np
import pytest
import torch

from oracle.modules import nt_xent_ref
from oracle.recipe import fill_module, probe
from tests import dropout_reference as dr
from tests.guard_bands import POISON, ZERO, guarded_ops, recording, same_bytes
from tests.test_clip_features_cpu import PS, ROW0S, SEED, SHAPES_RC, STEPS, TOWERS, make_x, overrides, write_tree
from tricolo_amd import config as tcfg
from tricolo_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tricolo_amd import ops
    from tricolo_amd.layers import CounterDropout
    from tricolo_amd.model.module.img_encoder.clip_img import CLIPImageEncoder
    from tricolo_amd.model.module.text_encoder.clip_text import CLIPTextEncoder
    from tricolo_amd.model.tricolo_net import TriCoLoNet

DEV = "cuda"
GPU_SHAPES = SHAPES_RC + [(257, 768)]
DROPOUT_ENTRY_POINTS = {"tri_dropout_tick", "tri_dropout_apply"}


@pytest.fixture(autouse=True)
def _precision():
    ops.set_default_precision("bf16x3")
    yield
    ops.set_default_precision("bf16x3")


def restated(x, p, seed, step, row0=0, tower=0):
    """ops.dropout_apply on host tensors: the torch restatement."""
    return ops.dropout_apply(x.cpu(), p, seed, torch.tensor([step], dtype=torch.int64), row0=row0, tower=tower)


# ---------------------------------------------------------------------------------------------------- the kernel
def kernel_grid(rows, cols, fill):
    """Every (row0, step, tower, p) of the CPU grid on one input, inside guard bands filled with `fill` -> {case: result on the host}."""
    x = make_x(rows, cols)
    out = {}
    with guarded_ops(fill) as g:
        xd = g.put(x)
        for step in STEPS:
            used = g.put(torch.tensor([step], dtype=torch.int64), origin="used")
            for row0 in ROW0S:
                for tower in TOWERS:
                    for p in PS:
                        out[(row0, step, tower, p)] = ops.dropout_apply(xd, p, SEED, used, row0=row0, tower=tower)
        assert g.launched == ["tri_dropout_apply"]
        out = {k: v.cpu() for k, v in out.items()}
    return x, out


@pytest.mark.parametrize("rows,cols", GPU_SHAPES, ids=[f"{r}x{c}" for r, c in GPU_SHAPES])
def test_kernel_equals_the_restatement_inside_guard_bands(rows, cols):
    x, poison = kernel_grid(rows, cols, POISON)
    _, zero = kernel_grid(rows, cols, ZERO)
    for (row0, step, tower, p), got in poison.items():
        want = restated(x, p, SEED, step, row0, tower)
        assert same_bytes(got, want), (rows, cols, row0, step, tower, p)
        assert same_bytes(got, zero[(row0, step, tower, p)])


@pytest.mark.parametrize("cols", [5, 6])
def test_kernel_on_row_offset_views(cols):
    """base[1:] of a [4, cols] tensor starts 4 * cols bytes into an aligned allocation: 4-byte aligned at cols = 5, 8-byte at cols = 6."""
    base = make_x(4, cols).to(DEV)
    x = base[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == (4 * cols) % 16
    used = torch.tensor([9], dtype=torch.int64, device=DEV)
    for p in PS:
        assert same_bytes(ops.dropout_apply(x, p, SEED, used, row0=4, tower=1).cpu(), restated(x, p, SEED, 9, 4, 1))
    assert torch.equal(base.cpu(), make_x(4, cols))


def test_kernel_on_a_misaligned_buffer_with_whole_groups():
    """cols % 4 == 0 but the pointer is only 4-byte aligned: the dword path, not the 16-byte one."""
    flat = torch.randn(1 + 7 * 8, generator=torch.Generator().manual_seed(3)).to(DEV)
    x = flat[1:].view(7, 8)
    assert x.data_ptr() % 16 == 4
    used = torch.tensor([2], dtype=torch.int64, device=DEV)
    assert same_bytes(ops.dropout_apply(x, 0.5, SEED, used).cpu(), restated(x, 0.5, SEED, 2))


def test_kernel_edge_values():
    x = make_x(8, 37)
    keep = dr.dropped(8, 37, 0.5, SEED, 5) == 0
    r, c = [int(v[0]) for v in np.nonzero(~keep)]
    rk, ck = [int(v[0]) for v in np.nonzero(keep)]
    x[r, c], x[rk, ck] = float("inf"), float("nan")
    used = torch.tensor([5], dtype=torch.int64, device=DEV)
    out = ops.dropout_apply(x.to(DEV), 0.5, SEED, used).cpu()
    assert torch.isnan(out[r, c]) and torch.isnan(out[rk, ck]) and int(torch.isnan(out).sum()) == 2      # inf * 0 = NaN
    assert same_bytes(out, restated(x, 0.5, SEED, 5))
    assert same_bytes(ops.dropout_apply(x.to(DEV), 0.0, SEED, used).cpu(), x)                            # p = 0: x exactly
    assert ops.dropout_apply(torch.zeros((0, 5), device=DEV), 0.1, SEED, used).shape == (0, 5)


def test_tick_semantics():
    """Two forwards draw steps s and s + 1; a backward reuses its own forward's step after a later forward has ticked; eval mode is
    the identity and launches nothing."""
    s = 2 ** 32 - 1                                                     # the low word wraps between the two forwards
    m = CounterDropout(0.1, tower=1, seed=SEED).to(DEV).train()
    m.step.fill_(s)
    x = make_x(8, 512).to(DEV).requires_grad_()
    with recording() as rec:
        y0 = m(x)
        y1 = m(x)
    assert rec.launches() == ["tri_dropout_tick", "tri_dropout_apply"] and rec.calls.count("tri_dropout_tick") == 2
    assert m.step.item() == s + 2
    up = make_x(8, 512, seed=1)
    (y0 * up.to(DEV)).sum().backward()
    assert same_bytes(y0.detach().cpu(), restated(x.detach(), 0.1, SEED, s, 0, 1))
    assert same_bytes(y1.detach().cpu(), restated(x.detach(), 0.1, SEED, s + 1, 0, 1))
    assert same_bytes(x.grad.cpu(), restated(up, 0.1, SEED, s, 0, 1))    # dx = dy * m of step s, not of s + 1
    assert not same_bytes(y0.detach().cpu(), y1.detach().cpu())
    m.eval()
    with recording() as rec:
        assert m(x) is x
    assert rec.calls == [] and m.step.item() == s + 2
    assert list(m.state_dict()) == []


def test_captured_step_draws_a_new_mask_on_every_replay():
    p, tower = 0.1, 1
    x, dy = make_x(8, 512).to(DEV), make_x(8, 512, seed=1).to(DEV)
    step = torch.tensor([40], dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # warm-up outside the capture, as torch asks for
        ops.dropout_apply(x, p, SEED, ops.dropout_tick(step), tower=tower)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        used = ops.dropout_tick(step)
        y = ops.dropout_apply(x, p, SEED, used, tower=tower)
        dx = ops.dropout_apply(dy, p, SEED, used, tower=tower)
    s = int(step.item())
    assert s == 41                                                       # the capture itself ran nothing
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(used.item()) == s + k and int(step.item()) == s + k + 1
        assert same_bytes(y.cpu(), restated(x, p, SEED, s + k, 0, tower)) and same_bytes(dx.cpu(), restated(dy, p, SEED, s + k, 0, tower))
        seen.append(y.cpu().clone())
    assert not same_bytes(seen[0], seen[1]) and not same_bytes(seen[1], seen[2])


# ---------------------------------------------------------------------------------------------------- the heads
def clip_batch(kind):
    batch = syn.make_batch(8, None, None, clip_img=kind == "img", clip_text=kind == "text", seed=syn.BASE_SEED + 5)
    return batch, batch[f"clip_embeddings_{kind}"]


def test_clip_image_encoder_eval_matches_reference(golden):
    from tests.test_gpu_modules import GRAD_RTOL, _check_grads, _sha
    g = golden("clip_img")
    m = CLIPImageEncoder(out_dim=512, num_views=6)
    fill_module(m, prefix="image_encoder.")
    m = m.to(DEV).eval()
    batch, x = clip_batch("img")
    assert _sha(x) == str(g["input_sha"])
    dbatch = syn.batch_to_device(batch, DEV)
    with recording() as rec:
        z = m(None, dbatch)
    assert not DROPOUT_ENTRY_POINTS & set(rec.calls)                     # eval mode launches no dropout kernel
    print("eval: max |z - reference|", float(np.abs(z.detach().cpu().numpy() - g["eval/z"]).max()))
    np.testing.assert_allclose(z.detach().cpu().numpy(), g["eval/z"], atol=2e-4)
    (z * torch.from_numpy(g["upstream"]).to(DEV)).sum().backward()
    _check_grads(m, g, "eval/", rtol=GRAD_RTOL, tag="clip_img_eval")
    with pytest.raises(UnboundLocalError):
        m(None, {})
    assert sorted(m.state_dict()) == [f"mlp.{i}.{w}" for i in (0, 3) for w in ("bias", "weight")]


def float64_head(module, x, mult, up):
    """Linear -> ReLU -> (* mult) -> Linear in float64 on the module's weights: (z, {parameter name: gradient})."""
    w0, b0, w1, b1 = (t.detach().cpu().double().requires_grad_() for t in (module.mlp[0].weight, module.mlp[0].bias, module.mlp[3].weight, module.mlp[3].bias))
    z = (torch.relu(x.double() @ w0.t() + b0) * mult) @ w1.t() + b1
    (z * up.double()).sum().backward()
    return z.detach(), {"mlp.0.weight": w0.grad, "mlp.0.bias": b0.grad, "mlp.3.weight": w1.grad, "mlp.3.bias": b1.grad}


def check_train_head(m, x, key, tower, up, tag):
    """One train-mode forward / backward of a CLIP head (dropout seed 123, step 0) against its float64 restatement with the counter mask."""
    mult = torch.from_numpy(dr.multiplier(8, 512, 0.1, 123, 0, 0, tower)).double()
    z = m(None, {key: x.to(DEV)})
    (z * up.to(DEV)).sum().backward()
    zr, grads = float64_head(m, x, mult, up)
    dz = float((z.detach().cpu().double() - zr).abs().max())
    dg = {n: float((p.grad.cpu().double() - grads[n]).abs().max()) for n, p in m.named_parameters()}
    print(f"{tag}: max |z - float64| {dz:.3e}; max |grad - float64| {dg}")
    np.testing.assert_allclose(z.detach().cpu().numpy(), zr.numpy(), atol=2e-5)
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[n].numpy(), atol=3e-5, rtol=2e-4, err_msg=n)
    assert int(m.mlp[2].step.item()) == 1
    return z, mult


def test_clip_image_encoder_train_matches_reference(golden):
    g = golden("clip_img")
    assert [int(g[f"train/mask_{k}"]) for k in ("seed", "step", "row0", "tower")] == [123, 0, 0, 1] and float(g["train/mask_p"]) == 0.1
    m = CLIPImageEncoder(out_dim=512, num_views=6, dropout_seed=123)
    fill_module(m, prefix="image_encoder.")
    m = m.to(DEV).train()
    _, x = clip_batch("img")
    z, mult = check_train_head(m, x, "clip_embeddings_img", 1, torch.from_numpy(g["upstream"]), "CLIPImageEncoder train")
    assert int((mult == 0).sum()) == int(g["train/mask_dropped"])
    # the fixture: the reference's own class in float64 with that mask in place of its Dropout
    np.testing.assert_allclose(z.detach().cpu().numpy(), g["train/z"], atol=2e-5)
    for n, p in m.named_parameters():
        norm, sample = probe(p.grad.cpu())
        ref_n, ref_s = float(g[f"train/gradnorm/{n}"]), g[f"train/gradsample/{n}"]
        np.testing.assert_allclose(sample, ref_s, atol=3e-5, rtol=2e-4, err_msg=n)
        assert abs(norm - ref_n) <= 3e-5 * np.sqrt(p.numel()) + 2e-4 * ref_n, (n, norm, ref_n)          # what the element bound allows the norm


def test_clip_text_encoder_counter_dropout_matches_float64():
    m = CLIPTextEncoder(out_dim=512, dropout="counter", dropout_seed=123)
    assert isinstance(m.mlp[2], CounterDropout) and m.mlp[2].tower == 0
    fill_module(m, prefix="text_encoder.")
    m = m.to(DEV).train()
    _, x = clip_batch("text")
    up = torch.randn((8, 512), generator=torch.Generator().manual_seed(7))
    check_train_head(m, x, "clip_embeddings_text", 0, up, "CLIPTextEncoder(dropout=counter) train")
    with pytest.raises(ValueError):
        CLIPTextEncoder(out_dim=512, dropout="philox")


# ---------------------------------------------------------------------------------------------------- training steps
BI_CLIP = ["data=synthetic", "model.text_encoder=CLIPTextEncoder", "model.image_encoder=CLIPImageEncoder", "model.voxel_encoder=null",
           "model.modules.CLIPTextEncoder.dropout=counter", "experiment_name=test"]


def test_four_adam_steps_match_a_float64_loop():
    from tests.test_gpu_modules import LOSS_TOL
    cfg = tcfg.compose(overrides=BI_CLIP)
    torch.manual_seed(123)                                               # the dropout seed of both heads
    net = TriCoLoNet(cfg)
    fill_module(net)
    assert [net.text_encoder.mlp[2].seed, net.image_encoder.mlp[2].seed] == [123, 123]
    # the float64 loop: two heads on the same recipe weights, oracle.modules.nt_xent_ref (text first: it is `zis`), torch.optim.Adam
    heads = {}
    for name, enc in (("text", net.text_encoder), ("image", net.image_encoder)):
        heads[name] = [t.detach().clone().double().requires_grad_() for t in (enc.mlp[0].weight, enc.mlp[0].bias, enc.mlp[3].weight, enc.mlp[3].bias)]
    ropt = torch.optim.Adam([t for h in heads.values() for t in h], lr=cfg.optimizer.lr, weight_decay=cfg.optimizer.weight_decay)
    batch = syn.make_batch(8, None, None, clip_text=True, clip_img=True, seed=syn.BASE_SEED + 5)
    xs = {"text": batch["clip_embeddings_text"].double(), "image": batch["clip_embeddings_img"].double()}
    net = net.to(DEV).train()
    dbatch = syn.batch_to_device(batch, DEV)
    assert "images" not in dbatch
    opt = net.configure_optimizers()
    report = []
    for step in range(4):
        opt.zero_grad(set_to_none=True)
        with recording() as rec:
            loss = net.training_step(dbatch, step)
            loss.backward()
            opt.step()
        if step == 0:
            print("entry points of a Bi(CLIP, CLIP) step:", rec.launches())
            assert DROPOUT_ENTRY_POINTS <= set(rec.launches())
        ropt.zero_grad(set_to_none=True)
        z = {}
        for tower, name in enumerate(("text", "image")):
            w0, b0, w1, b1 = heads[name]
            mult = torch.from_numpy(dr.multiplier(8, 512, 0.1, 123, step, 0, tower)).double()
            z[name] = (torch.relu(xs[name] @ w0.t() + b0) * mult) @ w1.t() + b1
        rloss = nt_xent_ref(z["text"], z["image"], cfg.loss.NTXentLoss.temperature, cfg.loss.NTXentLoss.alpha_weight)
        rloss.backward()
        ropt.step()
        report.append((loss.item(), rloss.item()))
    gaps = [abs(a - b) for a, b in report]
    print("Bi(CLIP, CLIP) losses (hip, float64):", report, "gaps:", gaps)
    assert all(np.isfinite(a) for a, _ in report)
    assert gaps[0] < LOSS_TOL, report
    for k in (1, 2, 3):
        assert gaps[k] < 1e-2, report
    assert report[-1][0] < report[0][0]                                  # and it trains
    assert [int(net.text_encoder.mlp[2].step.item()), int(net.image_encoder.mlp[2].step.item())] == [4, 4]


def test_bench_config_5_launches_no_dropout_kernel():
    """bench.py config 5 keeps CLIPTextEncoder on torch's dropout: one step of the net bench.py builds, under the recording wrapper."""
    import bench
    a = bench.parse_args(["--config", "5", "--per-gpu-batch", "2"])
    before = ops.default_precision()
    try:
        net, _ = bench.build_net(a, a.precision, DEV)
        assert isinstance(net.text_encoder.mlp[2], torch.nn.Dropout) and net.text_encoder.mlp[2].training
        batch = bench.make_batches(a, 0, DEV, 1)[0]
        opt = net.configure_optimizers()
        with recording() as rec:
            opt.zero_grad(set_to_none=True)
            loss = net.training_step(batch, 0)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
    finally:
        ops.set_default_precision(before)
    assert np.isfinite(loss.item()) and len(rec.launches()) > 20
    assert not DROPOUT_ENTRY_POINTS & set(rec.calls), rec.launches()


def test_train_and_test_commands_end_to_end(tmp_path):
    """python -m tricolo_amd.train for 2 epochs of Bi(CLIP image, CLIP text) on a packed tree without a single .npz, then
    python -m tricolo_amd.test on its last.ckpt: the metrics of the last validation, exactly."""
    import os
    from tricolo_amd import test as inference, train
    root = str(tmp_path / "exp_data")
    os.makedirs(root)
    write_tree(root, npz=False, dim=768)
    args = overrides(root, extra=["model.modules.CLIPTextEncoder.dropout=counter", "experiment_name=clip_e2e", f"experiment_output_path={tmp_path / 'out'}",
                                  "trainer.max_epochs=2", "trainer.check_val_every_n_epoch=1"])
    result = train.main(args)
    hist = result["history"]
    assert len(hist) == 2 and result["global_step"] == 6 and all(np.isfinite(h["train_loss"]) for h in hist)
    ckpt = tmp_path / "out" / "training" / "last.ckpt"
    assert ckpt.exists()
    sd = torch.load(ckpt, weights_only=False)["state_dict"]
    assert sorted(sd) == sorted(f"{t}.mlp.{i}.{w}" for t in ("text_encoder", "image_encoder") for i in (0, 3) for w in ("weight", "bias"))
    m = inference.main(args + [f"+ckpt_path={ckpt}"])
    assert float(m["recall_rate"][0] * 100) == hist[-1]["val_eval/RR@1"] and float(m["recall_rate"][4] * 100) == hist[-1]["val_eval/RR@5"]
    assert (tmp_path / "out" / "inference" / "val" / "predictions" / "output.p").exists()
