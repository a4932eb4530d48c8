#!/usr/bin/env python3
"""WavJEPA pre-training on MI355X: same wiring as the reference's train.py (registries, ComponentFactory, trainer
setup: reference train.py:21-35,47-130,160-206,225-250) on top of the HIP engine.

    python train.py                                   # configs/base.yaml
    python train.py masker=LibriSpeech trainer.steps=1000 trainer.batch_size=32
    python train.py data=audioset data.data_dirs=/path/to/shards data.device_prep=true    # resampling / loudness / padding on the GPU
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py trainer.num_gpus=8
"""
from __future__ import annotations

import os
import sys

import torch

from utils import checkpoint_dir, get_identity_from_cfg
from wavjepa_amd.config import load_config, parse_conv_spec
from wavjepa_amd.data import SyntheticAudioSource
from wavjepa_amd.extractors import ConvChannelFeatureExtractor, ConvFeatureExtractor, Extractor
from wavjepa_amd.jepa import JEPA
from wavjepa_amd.masking import SpeechMasker, TimeInverseBlockMasker
from wavjepa_amd.trainer import Trainer
from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG

NETWORKS = {"JEPA": JEPA}
MASKERS = {"time-inverse": TimeInverseBlockMasker, "speech-masker": SpeechMasker}
EXTRACTORS = {"wav2vec2": ConvFeatureExtractor, "wavjepa": ConvFeatureExtractor,
              # BASELINE config 4 (WavJEPA-Nat): the reference's registry (train.py:26-29) never selects its channel extractor; this one does
              "wavjepa-nat": ConvChannelFeatureExtractor}


class ComponentFactory:
    @staticmethod
    def create_extractor(cfg) -> Extractor:
        cls = EXTRACTORS.get(cfg.extractor.name)
        if cls is None:
            raise ValueError(f"Unknown extractor type: {cfg.extractor.name}. Available extractors: {list(EXTRACTORS.keys())}")
        norm = dict(mode=str(cfg.extractor.get("mode", "default")), conv_bias=bool(cfg.extractor.get("conv_bias", False)))
        if cls is ConvChannelFeatureExtractor:
            return cls(conv_layers_spec=parse_conv_spec(cfg.extractor.conv_layers_spec), in_channels=cfg.data.in_channels,
                       share_weights_over_channels=bool(cfg.extractor.get("share_weights_over_channels", False)), **norm)
        return cls(conv_layers_spec=parse_conv_spec(cfg.extractor.conv_layers_spec), in_channels=cfg.data.in_channels,
                   depthwise=cfg.extractor.depthwise, **norm)

    @staticmethod
    def create_masker(cfg):
        cls = MASKERS.get(cfg.masker.name)
        if cls is None:
            raise ValueError(f"Unknown masker type: {cfg.masker.name}. Available maskers: {list(MASKERS.keys())}")
        mk = cfg.masker
        if mk.name == "speech-masker":
            return SpeechMasker(target_masks_per_context=mk.target_masks_per_context, target_prob=mk.target_prob,
                                target_length=mk.target_length, ratio_cutoff=mk.ratio_cutoff,
                                channel_based_masking=mk.channel_based_masking, min_context_len=mk.min_context_len)
        # the reference reads cfg.masker.context_prob / context_length while its YAML spells context_mask_prob /
        # context_mask_length (SURVEY §5 drift 1): accept both spellings.
        prob = mk.get("context_prob", mk.get("context_mask_prob"))
        length = mk.get("context_length", mk.get("context_mask_length"))
        return TimeInverseBlockMasker(target_masks_per_context=mk.target_masks_per_context, context_mask_prob=prob,
                                      context_mask_length=length, target_prob=mk.target_prob, target_length=mk.target_length,
                                      ratio_cutoff=mk.ratio_cutoff, channel_based_masking=mk.channel_based_masking,
                                      channel_major=bool(mk.get("channel_major", False)))

    @staticmethod
    def create_network(cfg, extractor: Extractor) -> JEPA:
        cls = NETWORKS.get(cfg.model)
        if cls is None:
            raise ValueError(f"Unknown network type: {cfg.model}. Available networks: {list(NETWORKS.keys())}")
        # trainer.norm_first: pre-norm layers in every stack; trainer.norm_first_decoder: the predictor's own setting (default: the same)
        norm_first = bool(cfg.trainer.get("norm_first", False))
        norm_first_dec = bool(cfg.trainer.get("norm_first_decoder", norm_first))
        # trainer.dropout_encoder / trainer.dropout_decoder: dropout of the student's / the predictor's layers in training (default 0)
        drop_enc, drop_dec = float(cfg.trainer.get("dropout_encoder", 0.0)), float(cfg.trainer.get("dropout_decoder", 0.0))
        # trainer.loss: the per-element objective on target rows; trainer.loss_beta: smooth-L1's beta / Huber's delta
        loss, beta = str(cfg.trainer.get("loss", "mse")), float(cfg.trainer.get("loss_beta", 1.0))
        losses = {"mse": lambda: None, "l1": lambda: torch.nn.L1Loss(reduction="none"),
                  "smooth_l1": lambda: torch.nn.SmoothL1Loss(reduction="none", beta=beta),
                  "huber": lambda: torch.nn.HuberLoss(reduction="none", delta=beta)}
        if loss not in losses:
            raise ValueError(f"Unknown trainer.loss: {loss}. Available losses: {list(losses)}")
        # trainer.activation: the feed-forward activation of every stack (gelu | gelu_tanh | relu | silu); trainer.activation_decoder: the
        # predictor's own (default: the same)
        act = str(cfg.trainer.get("activation", "gelu"))
        act_dec = str(cfg.trainer.get("activation_decoder", act))
        acts = {"gelu": lambda: None, "gelu_tanh": lambda: torch.nn.GELU(approximate="tanh"), "relu": torch.nn.ReLU, "silu": torch.nn.SiLU}
        for key, a in (("trainer.activation", act), ("trainer.activation_decoder", act_dec)):
            if a not in acts:
                raise ValueError(f"Unknown {key}: {a}. Available activations: {list(acts)}")
        try:
            return cls(**optimizer_group_settings(cfg), **layerdrop_settings(cfg), **freeze_settings(cfg), feature_extractor=extractor, transformer_encoder_cfg=TransformerEncoderCFG.create(),
                       transformer_encoder_layers_cfg=TransformerLayerCFG.create(norm_first=norm_first, dropout=drop_enc, activation=acts[act]()),
                       transformer_decoder_cfg=TransformerEncoderCFG.create(),
                       transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384, norm_first=norm_first_dec, dropout=drop_dec,
                                                                                 activation=acts[act_dec]()),
                       lr=cfg.optimizer.lr,
                       adam_betas=(cfg.optimizer.b1, cfg.optimizer.b2), adam_weight_decay=cfg.optimizer.weight_decay,
                       resample_sr=cfg.data.sr, process_audio_seconds=cfg.data.process_seconds,
                       nr_samples_per_audio=cfg.data.samples_per_audio, compile_modules=cfg.trainer.compile_modules,
                       average_top_k_layers=cfg.trainer.average_top_k_layers, size=cfg.trainer.get("size", "base"),
                       warmup_steps=cfg.trainer.get("warmup_steps", 100000), loss_fn=losses[loss](),
                       # trainer.use_gradient_checkpointing: recompute layer activations in the backward (student and predictor)
                       use_gradient_checkpointing=bool(cfg.trainer.get("use_gradient_checkpointing", False)))
        except Exception as e:
            raise RuntimeError(f"Failed to create network instance: {str(e)}")


def optimizer_group_settings(cfg) -> dict:
    """The model keywords that give the optimiser parameter groups, only those that are set (so a default run builds the model it always
    built): optimizer.weight_decay_exclude (`1d`, or a list of fnmatch patterns on parameter names: those go without weight decay) and
    optimizer.layer_lr_decay (BEiT's layer-wise lr decay; 1.0 = none)."""
    exclude = cfg.optimizer.get("weight_decay_exclude", None)
    decay = float(cfg.optimizer.get("layer_lr_decay", 1.0))
    kw = {}
    if exclude is not None:
        kw["weight_decay_exclude"] = exclude if isinstance(exclude, str) else tuple(str(x) for x in exclude)
    if decay != 1.0:
        kw["layer_lr_decay"] = decay
    return kw


def layerdrop_settings(cfg) -> dict:
    """The model keywords of LayerDrop, only those that are set: trainer.encoder_layerdrop / trainer.decoder_layerdrop, the probability
    with which a training step skips each layer of the student / the predictor (default 0: every layer runs)."""
    kw = {}
    for key in ("encoder_layerdrop", "decoder_layerdrop"):
        p = float(cfg.trainer.get(key, 0.0))
        if p != 0.0:
            kw[key] = p
    return kw


def freeze_settings(cfg) -> dict:
    """The model keywords of partial training, only those that are set: trainer.feature_grad_mult (fairseq's factor on the gradient that
    enters the conv stack, in [0, 1]; default 1) and trainer.freeze_feature_extractor_updates (optimiser steps during which
    extract_audio.* stays frozen; default 0).  trainer.freeze, a list of fnmatch patterns on parameter names, is applied to the built
    model (build_model) and recorded with them."""
    kw = {}
    mult = float(cfg.trainer.get("feature_grad_mult", 1.0))
    if mult != 1.0:
        kw["feature_grad_mult"] = mult
    hold = int(cfg.trainer.get("freeze_feature_extractor_updates", 0) or 0)
    if hold != 0:
        kw["freeze_feature_extractor_updates"] = hold
    return kw


def freeze_patterns(cfg) -> tuple:
    pats = cfg.trainer.get("freeze", None)
    if pats is None or isinstance(pats, str) and not pats:
        return ()
    if isinstance(pats, str) and pats.startswith("[") and pats.endswith("]"):      # trainer.freeze=[extract_audio.*,*.bias] on the command line
        pats = [p.strip().strip("'\"") for p in pats[1:-1].split(",") if p.strip()]
    return (pats,) if isinstance(pats, str) else tuple(str(p) for p in pats)


def monitor_settings(cfg) -> tuple:
    """(monitor_every, min_pred_var, min_target_var): trainer.monitor_every steps between two collapse monitors (0 = off, the default),
    trainer.min_pred_var / trainer.min_target_var the thresholds below which the run stops (0 = no check; data2vec 2.0: 0.01 / 0.1).
    A threshold without monitor_every monitors the steps the trainer logs."""
    every = int(cfg.trainer.get("monitor_every", 0))
    min_pred, min_target = float(cfg.trainer.get("min_pred_var", 0.0)), float(cfg.trainer.get("min_target_var", 0.0))
    if every == 0 and (min_pred > 0 or min_target > 0):
        every = int(cfg.trainer.get("log_every_n_steps", 50))
    return every, min_pred, min_target


def setup_trainer(cfg) -> Trainer:
    _, min_pred, min_target = monitor_settings(cfg)
    return Trainer(min_pred_var=min_pred, min_target_var=min_target, accelerator=cfg.trainer.accelerator, max_epochs=cfg.trainer.epochs, max_steps=cfg.trainer.steps,
                   precision=cfg.trainer.precision, devices=int(cfg.trainer.num_gpus), gradient_clip_val=5,
                   gradient_clip_algorithm="norm", strategy="ddp" if int(cfg.trainer.num_gpus) > 1 else "auto",
                   log_every_n_steps=cfg.trainer.get("log_every_n_steps", 50),
                   deterministic=bool(cfg.trainer.get("deterministic", False)),     # the reference passes deterministic=False (train.py:170)
                   # trainer.accumulate_grad_batches: loader batches per optimiser step (pl.Trainer's argument; default 1)
                   accumulate_grad_batches=cfg.trainer.get("accumulate_grad_batches", 1),
                   checkpoint_every_n_steps=25000,      # ModelCheckpoint(every_n_train_steps=25000, save_last=True), reference train.py:146-153
                   default_root_dir=checkpoint_dir(cfg, "saved_models_jepa_new_masking", get_identity_from_cfg(cfg)))


def build_model(cfg):
    extractor = ComponentFactory.create_extractor(cfg)
    network = ComponentFactory.create_network(cfg, extractor)
    if hasattr(network, "monitor_every"):
        network.monitor_every = monitor_settings(cfg)[0]
    patterns = freeze_patterns(cfg)
    if patterns:                 # trainer.freeze: recorded in the checkpoint's hyper-parameters, only when set
        network.freeze(*patterns)
        network.hparams["freeze"] = patterns
    return network, extractor.total_patches(int(cfg.data.sr * cfg.data.process_seconds))


def create_data_source(cfg, nr_patches, device, rank):
    masker = ComponentFactory.create_masker(cfg)
    if cfg.data.name == "NatSynthetic":     # BASELINE config 4: binaural scenes generated on the device inside the step
        from wavjepa_amd.data import NatSceneSource
        if int(cfg.data.in_channels) != 2:
            raise ValueError("data=nat_synthetic produces 2-channel scenes: data.in_channels must be 2")
        return NatSceneSource(masker, batch_size=cfg.trainer.batch_size, samples_per_audio=cfg.data.samples_per_audio, n_tokens=nr_patches,
                              sr=cfg.data.sr, seconds=cfg.data.get("source_seconds", 10.0), rir_seconds=cfg.data.get("rir_seconds", 0.5),
                              n_noise=int(cfg.data.get("n_noise", 2)), seed=cfg.seed + rank, device=device)
    if cfg.data.name != "Synthetic":        # tar shards of .flac clips (reference train.py:94-110 -> data_modules/WebAudioDataModule.py)
        from wavjepa_amd.data_modules import WebAudioDataModule
        dm = WebAudioDataModule(masker, data_dirs=cfg.data.data_dirs, mixing_weights=cfg.data.get("mixing_weights", None),
                                batch_size=cfg.trainer.batch_size, nr_samples_per_audio=cfg.data.samples_per_audio,
                                nr_time_points=nr_patches, in_channels=cfg.data.in_channels, sr=cfg.data.sr, seed=cfg.seed, rank=rank,
                                world_size=cfg.trainer.num_gpus, device_prep=bool(cfg.data.get("device_prep", False)), prep_device=device)
        dm.setup("fit")
        return dm.train_dataloader()
    return SyntheticAudioSource(masker, batch_size=cfg.trainer.batch_size, samples_per_audio=cfg.data.samples_per_audio,
                                n_tokens=nr_patches, in_channels=cfg.data.in_channels, sr=cfg.data.sr,
                                seconds=cfg.data.get("source_seconds", 10.0), seed=cfg.seed + rank, device=device)


def main(argv=None):
    cfg = load_config(os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs"), list(argv if argv is not None else sys.argv[1:]))
    try:
        torch.manual_seed(cfg.seed)
        trainer = setup_trainer(cfg)
        model, patches = build_model(cfg)
        device = torch.device("cuda", trainer.local_rank)
        if trainer.deterministic:
            # a repeatable run also needs repeatable masks: the synthetic sources draw their mask sets once, here, from seeded generators
            # (the maskers otherwise use OS entropy, as upstream; shard loaders draw per batch in their workers and are not pinned)
            from wavjepa_amd.data import pinned_mask_draws
            with pinned_mask_draws(int(cfg.seed) + trainer.rank):
                source = create_data_source(cfg, patches, device, trainer.rank)
        else:
            source = create_data_source(cfg, patches, device, trainer.rank)
        if trainer.rank == 0:
            print(f"Effective Batch Size is: "
                  f"{cfg.trainer.batch_size * cfg.data.samples_per_audio * cfg.trainer.num_gpus * trainer.accumulate_grad_batches}")
        trainer.fit(model, train_dataloaders=source)
    except Exception as e:
        print(f"Training failed with error: {str(e)}")
        raise


if __name__ == "__main__":
    main()
