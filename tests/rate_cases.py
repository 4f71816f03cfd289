"""What the mixed-rate tests share (not a test module): a tiny three-rate model whose rate indices differ strongly, and a clip of
three intra-period units of different sizes.

Model: FullNet with arch.TINY_WIDTHS and nb_rates = 3, seeded as tests/test_gpu_codec.py::test_fractional_rate_index_matches_oracle
does; then every gain matrix is overwritten: encoder gain of index i = 2^i x (1 + jitter), jitter uniform in [0, 0.05) from a seeded
generator, decoder gain = its reciprocal.  Index 2 is the rich end (about twice the bytes of index 0).

Clip: 9 frames of 64 x 48 coded as 1_GOP_2, i.e. three units of three frames; unit u is synth.synthetic_video(seed=4) with noise
NOISE[u].  GOP records of the three units at rate index 0 and 2 (the same on the device and in the CPU oracle): 315 and 650, 309 and
680, 363 and 764 bytes; TARGET_BPP = 0.43 is a budget of 495 bytes per unit, between every unit's lean and rich end, and the three
units end on three different rate indices (1.3125 with 493 bytes, 1.125 with 490, 0.75 with exactly 495)."""
import torch

W, H, GOP, UNIT = 64, 48, '1_GOP_2', 3
NOISE = (0.0, 25.0, 120.0)
LAMBDAS = [0.01, 0.02, 0.04]
NB_RATES = 3
TARGET_BPP = 0.43


def make_model(device=None, coders=True):
    from aivc_amd import synth
    from aivc_amd.model_mngt.model_management import attach_arithmetic_coders
    from aivc_amd.models import arch
    from aivc_amd.models.full_net import FullNet
    torch.manual_seed(5)
    model = FullNet({'widths': arch.TINY_WIDTHS, 'nb_rates': NB_RATES, 'lambda_tradeoff': list(LAMBDAS)})
    synth._init_weights(model, torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for net in (model.mode_net.mode_net, model.codec_net.codec_net):
            for gm in (net.gain_I, net.gain_P, net.gain_B):
                for i in range(NB_RATES):
                    enc = (2.0 ** i) * (1 + 0.05 * torch.rand(gm.enc_gain_list[i].shape, generator=gen))
                    gm.enc_gain_list[i].copy_(enc)
                    gm.dec_gain_list[i].copy_(1.0 / enc)
    model = model.eval()
    if device is not None:
        model = model.to(device)
    return attach_arithmetic_coders(model) if coders else model


def unit_frames(u):
    """the three frames of unit u (numpy planes)"""
    from aivc_amd import synth
    return synth.synthetic_video(W, H, UNIT, seed=4, noise=NOISE[u])


def clip():
    return [f for u in range(len(NOISE)) for f in unit_frames(u)]
