"""The layer-norm wav2vec2 architecture (feat_extract_norm="layer", conv_bias=True,
do_stable_layer_norm=True: XLSR-53, XLS-R, the -lv60 family) on the HIP kernels vs transformers'
Wav2Vec2Model.

* mini dims: against the committed float64 golden (tests/golden/make_w2v2_ln_golden.py): hidden
  states and every parameter gradient of Σ(hidden·cot), with and without a sample mask;
* large dims (hidden 1024, 16 heads, intermediate 4096, 7 x 512 convs with bias + LayerNorm, 2
  layers, 1 s clips, B = 2): against transformers run live in fp32 on the same GPU, same weights;
* a TrainStep on raw waveforms through the public EnhancedAudioTextModel: finite loss, every
  trainable audio parameter moves, a second identically seeded run is bitwise equal;
* the eval forward with and without saved activations.
Bounds and error measures are those of this encoder family in tests/test_w2v2_gpu.py, imported."""
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_w2v2_gpu import GRAD_TOL, HID_TOL, _grad_errors, _model, _rel

pytestmark = pytest.mark.gpu
sys.path.insert(0, str(GOLDEN))

LN = dict(feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True)


def _mini():
    from speech_transcript_embeddings_amd.modules import W2V2Config
    return W2V2Config(**json.loads((GOLDEN / "w2v2_ln_golden.json").read_text())["config"])


@pytest.fixture(scope="module")
def golden():
    import make_w2v2_ln_golden as mk
    return mk.load()


def _load_golden(m, golden):
    sd = {k[len("param/"):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("param/")}
    m.audio_encoder.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("case", ["mask", "nomask"])
def test_mini_matches_transformers_golden(golden, case):
    m = _model(_mini())
    _load_golden(m, golden)
    wave = torch.from_numpy(golden[f"{case}/wave"]).cuda()
    mask = torch.from_numpy(golden[f"{case}/mask"]).cuda() if f"{case}/mask" in golden else None
    m.zero_grad(set_to_none=True)
    _, hidden = m.encode_audio(wave, mask)
    ref_h = golden[f"{case}/hidden"]
    assert hidden.shape == ref_h.shape
    e_h = _rel(hidden.detach().cpu().numpy(), ref_h)
    print(f"{case}: hidden {e_h:.3e}")
    assert e_h < HID_TOL, e_h
    cot = torch.from_numpy(golden[f"{case}/cot"]).cuda()
    (hidden * cot).sum().backward()
    torch.cuda.synchronize()
    params = dict(m.audio_encoder.named_parameters())
    pre = f"{case}/grad/"
    ref = {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}
    assert all(params[n].grad is not None for n in ref)
    errs = _grad_errors({n: params[n].grad.cpu().numpy() for n in ref}, ref)
    print(f"{case}: worst gradients", sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    bad = {n: e for n, e in errs.items() if not e < GRAD_TOL}
    assert not bad, bad
    assert len(errs) == len(params)


def test_large_dims_match_transformers_live():
    """XLSR shapes (2 layers) against transformers fp32 on the GPU, same weights."""
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    from speech_transcript_embeddings_amd.modules import W2V2Config
    kw = dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=2,
              hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0,
              mask_time_prob=0.0, **LN)
    torch.manual_seed(0)
    hf = Wav2Vec2Model(Wav2Vec2Config(**kw, attn_implementation="eager")).cuda().train()
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(1)
        for n, p in hf.named_parameters():
            if n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, device="cuda", generator=g))
    m = _model(W2V2Config(**kw))
    m.audio_encoder.load_state_dict({k: v.detach().float() for k, v in hf.state_dict().items()}, strict=True)
    B, N = 2, 16000
    gen = torch.Generator(device="cuda").manual_seed(2)
    wave = torch.randn(B, N, device="cuda", generator=gen)
    mask = torch.ones(B, N, dtype=torch.int64, device="cuda")
    mask[1, 11000:] = 0
    wave[1, 11000:] = 0
    ref = hf(input_values=wave, attention_mask=mask).last_hidden_state
    _, hid = m.encode_audio(wave, mask)
    assert hid.shape == ref.shape
    e_h = _rel(hid.detach().cpu().numpy(), ref.detach().cpu().numpy())
    print(f"large dims: hidden {e_h:.3e}")
    assert e_h < HID_TOL, e_h
    cot = torch.randn(ref.shape, device="cuda", generator=gen)
    (ref * cot).sum().backward()
    m.zero_grad(set_to_none=True)
    (hid * cot).sum().backward()
    ours = dict(m.audio_encoder.named_parameters())
    ref = {n: p.grad.cpu().numpy() for n, p in hf.named_parameters() if p.grad is not None}
    assert len(ref) == len(ours)
    errs = _grad_errors({n: ours[n].grad.cpu().numpy() for n in ref}, ref)
    print("large dims: worst gradients", sorted(errs.items(), key=lambda kv: -kv[1])[:5])
    bad = {n: e for n, e in errs.items() if not e < GRAD_TOL}
    assert not bad, bad


def _train_once():
    """One optimizer-moving TrainStep sequence (two calls: the warmup's first factor is 0) with the
    default dropout / layerdrop / SpecAugment probabilities -> (losses, audio parameters before/after)."""
    from speech_transcript_embeddings_amd.model import EnhancedAudioTextModel
    from speech_transcript_embeddings_amd.modules import TextConfig, W2V2Config
    from speech_transcript_embeddings_amd.train import TrainStep
    torch.manual_seed(5)      # dropout seeds
    np.random.seed(5)         # SpecAugment's span sampling
    tc = TextConfig(vocab_size=512, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                    max_position_embeddings=66)
    cfg = json.loads((GOLDEN / "w2v2_ln_golden.json").read_text())["config"]
    cfg.update(hidden_dropout=0.1, activation_dropout=0.1, attention_dropout=0.1, layerdrop=0.0, mask_time_prob=0.05)
    m = EnhancedAudioTextModel(text_model_name=tc, audio_model_name=W2V2Config(**cfg), projection_dim=64,
                               text_embedding_dim=64, audio_embedding_dim=64, freeze_encoders="partial",
                               text_layers_to_unfreeze=1, audio_layers_to_unfreeze=1, device="cuda").train()
    step = TrainStep(m, gather_embeddings=False)
    B, N, L = 4, 4000, 12
    g = torch.Generator(device="cuda").manual_seed(3)
    wav = torch.randn(B, N, device="cuda", generator=g)
    lengths = torch.tensor([4000, 3500, 3000, 2600], device="cuda", dtype=torch.int32)
    ids = torch.randint(3, 500, (B, L), device="cuda", generator=g)
    am = torch.ones(B, L, dtype=torch.int64, device="cuda")
    before = {n: p.detach().clone() for n, p in m.audio_encoder.named_parameters()}
    losses = [float(step(wav, lengths, ids, am, ids.flip(0), am)) for _ in range(2)]
    after = {n: p.detach().clone() for n, p in m.audio_encoder.named_parameters()}
    trainable = {n for n, p in m.audio_encoder.named_parameters() if p.requires_grad}
    return losses, before, after, trainable


def test_train_step_on_raw_waveforms():
    """TrainStep through the public model, last audio layer unfrozen (the conv stack, positional conv,
    feature projection and trailing LayerNorm are never frozen): finite losses, every trainable audio
    parameter moves, frozen ones do not, and an identically seeded second run is bitwise equal."""
    losses, before, after, trainable = _train_once()
    assert all(np.isfinite(l) for l in losses), losses
    frozen = set(before) - trainable
    assert any(n.startswith("encoder.layers.0.") for n in frozen) and "encoder.layers.1.layer_norm.weight" in trainable
    # the key-projection bias has an exactly zero gradient (softmax ignores a per-query shift)
    still = {n for n in trainable if torch.equal(before[n], after[n]) and not n.endswith("k_proj.bias")}
    assert not still, sorted(still)
    assert all(torch.isfinite(after[n]).all() for n in after)
    assert all(torch.equal(before[n], after[n]) for n in frozen)
    losses2, _, after2, _ = _train_once()
    assert losses2 == losses
    assert all(torch.equal(after[n], after2[n]) for n in after)


def test_eval_forward_without_saved_activations(golden):
    """Eval mode: the forward-only path (no_grad: save=False) against the saving forward.  The two
    are not bitwise equal by design: without a backward to feed, attention multiplies P·V on bf16 P
    instead of the hi/lo split (tests/test_eval_gpu.py), so they agree to that test's bound, 5e-3
    relative L2 — and the forward-only result meets the golden's bound on its own."""
    m = _model(_mini()).eval()
    _load_golden(m, golden)
    wave = torch.from_numpy(golden["mask/wave"]).cuda()
    mask = torch.from_numpy(golden["mask/mask"]).cuda()
    _, h_save = m.encode_audio(wave, mask)
    with torch.no_grad():
        _, h_nosave = m.encode_audio(wave, mask)
    assert h_save.requires_grad and not h_nosave.requires_grad
    assert h_save.shape == h_nosave.shape
    e = _rel(h_nosave.cpu().numpy(), h_save.detach().cpu().numpy())
    print(f"save=False vs save=True: {e:.3e}")
    assert e < 5e-3, e
    assert _rel(h_nosave.cpu().numpy(), golden["mask/hidden"]) < HID_TOL
