"""-m gpu: `from_pretrained(<dir>)` and the encoder half of the checkpoint's VAE: built (strictly loaded) when the safetensors hold
`encoder.*` tensors, `pipe.vae_encoder is None` when they do not, and the loaded encoder gives the bits of an engine loaded by hand."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _write(tmp_path, with_encoder):
    from safetensors.torch import save_file
    from diffmusic_amd import checkpoint as ck
    from diffmusic_amd.engine import HifiGanEngine, UNetEngine, VaeDecoderEngine, VaeEncoderEngine
    from tests.test_checkpoint_config import UNET_MUSICLDM, VAE as VAE_JSON, VOCODER
    ucfg = dict(UNET_MUSICLDM, block_out_channels=[32, 64, 96, 160])
    ucfg["cross_attention_dim"] = [32, 64, 96, 160]
    vcfg = dict(VAE_JSON, block_out_channels=[32, 64, 64])
    hcfg = dict(VOCODER, upsample_initial_channel=128)
    enc_sd = None
    for k, (sub, cfg, fn, Eng) in enumerate((("unet", ucfg, ck.unet_config, UNetEngine), ("vae", vcfg, ck.vae_config, VaeDecoderEngine),
                                             ("vocoder", hcfg, ck.vocoder_config, HifiGanEngine))):
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "config.json", "w") as fh:
            json.dump(cfg, fh)
        sd = Eng(fn(cfg)).synth_state_dict(seed=k)
        if sub == "vae" and with_encoder:
            enc_sd = VaeEncoderEngine(fn(cfg)).synth_state_dict(seed=9)
            sd = dict(sd, **enc_sd)
        save_file({n: v.contiguous() for n, v in sd.items()}, str(tmp_path / sub / "diffusion_pytorch_model.safetensors"))
    return ck.vae_config(vcfg), enc_sd


def test_checkpoint_with_the_encoder_half_loads_it(tmp_path):
    from diffmusic_amd.engine import VaeEncoderEngine
    from diffmusic_amd.pipelines import get_pipeline
    vcfg, enc_sd = _write(tmp_path, True)
    pipe = get_pipeline("musicldm").from_pretrained(str(tmp_path)).to("cuda")
    assert isinstance(pipe.vae_encoder, VaeEncoderEngine) and pipe.vae_encoder.cfg["block_out_channels"] == [32, 64, 64]
    ref = VaeEncoderEngine(vcfg).load_state_dict(enc_sd, strict=True)
    mel = (2.0 * torch.randn(2, 40, 64, generator=torch.Generator().manual_seed(2)) - 4.0).cuda()
    assert torch.equal(pipe.vae_encoder.encode_hip(mel), ref.encode_hip(mel))


def test_checkpoint_without_the_encoder_half_has_none(tmp_path):
    from diffmusic_amd.pipelines import get_pipeline
    _write(tmp_path, False)
    pipe = get_pipeline("musicldm").from_pretrained(str(tmp_path)).to("cuda")
    assert pipe.vae_encoder is None
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_step import SCHED
    pipe.scheduler = get_scheduler("ddim")(operator=P.IdentityOperator(16000), **SCHED)
    pipe.assume_uncond_equals_cond = True
    with pytest.raises(ValueError, match="vae_encoder"):
        pipe(prompt_embeds=torch.zeros(1, 512), audio_length_in_s=0.4, num_inference_steps=4, show_progress=False,
             init_mel=torch.zeros(1, 40, 64), strength=0.5)
