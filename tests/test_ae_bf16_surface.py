"""CPU checks of BasicAE's precision switch: the flag, its validation, checkpoints across modes, what a fine-tuning module
inherits, and the refusal of the BatchNorm2d variants (no GPU needed: nothing here launches a kernel)."""
from argparse import ArgumentParser, Namespace

import pytest

HP = dict(hidden_dim=16, latent_dim=8, input_height=16, input_width=132, output_height=16, output_width=22)


def _ae(**kw):
    from driving_dirty_amd.autoencoder import BasicAE
    return BasicAE(Namespace(**HP, **kw))


def test_precision_flag_is_parsed_with_its_choices():
    from driving_dirty_amd.autoencoder import BasicAE
    parser = BasicAE.add_model_specific_args(ArgumentParser(add_help=False))
    assert parser.parse_args([]).precision == "fp32"
    assert parser.parse_args(["--precision", "bf16"]).precision == "bf16"
    with pytest.raises(SystemExit):
        parser.parse_args(["--precision", "fp16"])


def test_default_is_fp32_and_unknown_precision_raises():
    ae = _ae()
    assert ae.precision == "fp32" and ae.encoder.precision == "fp32" and ae.decoder.precision == "fp32"
    ae = _ae(precision="bf16")
    assert ae.precision == "bf16" and ae.encoder.precision == "bf16" and ae.decoder.precision == "bf16"
    with pytest.raises(ValueError):
        _ae(precision="fp16")
    with pytest.raises(ValueError):
        ae.precision = "tf32"
    assert ae.precision == "bf16"


def test_state_dict_is_the_same_in_both_modes_and_loads_across():
    import torch
    torch.manual_seed(0)
    a32 = _ae()
    torch.manual_seed(0)
    a16 = _ae(precision="bf16")
    s32, s16 = a32.state_dict(), a16.state_dict()
    assert list(s32) == list(s16)
    assert not any("precision" in k for k in s16)
    assert all(torch.equal(s32[k], s16[k]) for k in s32)      # same RNG consumption: same initial weights
    with torch.no_grad():
        for p in a32.parameters():
            p.add_(1.0)
    a16.load_state_dict(a32.state_dict())
    a32.load_state_dict(a16.state_dict())
    assert a16.precision == "bf16" and a32.precision == "fp32"
    assert all(torch.equal(a32.state_dict()[k], a16.state_dict()[k]) for k in s32)


def test_checkpoint_round_trip_keeps_the_precision(tmp_path):
    from driving_dirty_amd.autoencoder import BasicAE
    ae = _ae(precision="bf16", learning_rate=1e-3)
    path = str(tmp_path / "ae.ckpt")
    ae.save_checkpoint(path)
    back = BasicAE.load_from_checkpoint(path)
    assert back.precision == "bf16" and back.decoder.precision == "bf16"


def test_roadmap_inherits_bf16_from_the_pretrained_ae_unless_overridden():
    from driving_dirty_amd.roadmap import RoadMapBCE
    hp = dict(unfreeze_epoch_no=0, learning_rate=1e-3, output_img_freq=500)
    model = RoadMapBCE(Namespace(pretrained_ae=_ae(precision="bf16"), **hp))
    assert model.ae.encoder.precision == "bf16"
    model = RoadMapBCE(Namespace(pretrained_ae=_ae(precision="bf16"), precision="fp32", **hp))
    assert model.ae.encoder.precision == "fp32"
    model = RoadMapBCE(Namespace(pretrained_ae=_ae(), **hp))
    assert model.ae.encoder.precision == "fp32"


def test_batchnorm_variants_refuse_bf16():
    from driving_dirty_amd import components_v2
    from driving_dirty_amd.autoencoder import BasicAE

    class BasicAEV2(BasicAE):
        def init_encoder(self, hidden_dim, latent_dim, in_channels, input_height, input_width):
            return components_v2.Encoder(hidden_dim, latent_dim, in_channels, input_height, input_width)

        def init_decoder(self, hidden_dim, latent_dim, in_channels, output_height, output_width):
            return components_v2.Decoder(hidden_dim, latent_dim, in_channels, output_height, output_width)

    ae = BasicAEV2(Namespace(**HP))
    assert ae.precision == "fp32" and ae.encoder.precision == "fp32"
    with pytest.raises(ValueError, match="only precision 'fp32'"):
        BasicAEV2(Namespace(precision="bf16", **HP))
    with pytest.raises(ValueError):
        ae.decoder.precision = "bf16"


def test_spatial_model_inherits_bf16_from_the_pretrained_ae_unless_overridden():
    """BBSpatialRoadMap takes its default precision from the AE's encoder too (spatial.py): a bf16 AE gives a bf16 encoder."""
    from driving_dirty_amd.spatial import BBSpatialRoadMap
    hp = dict(unfreeze_epoch_no=10 ** 9, learning_rate=1e-3, output_img_freq=500)
    model = BBSpatialRoadMap(Namespace(pretrained_ae=_ae(precision="bf16"), **hp))
    assert model.ae.encoder.precision == "bf16"
    model = BBSpatialRoadMap(Namespace(pretrained_ae=_ae(precision="bf16"), precision="fp32", **hp))
    assert model.ae.encoder.precision == "fp32"
