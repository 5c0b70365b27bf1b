"""vae_model_fn -- same (features, labels, mode, params) contract as the reference (src/model_fns_tf.py:9-114):
builds the DiscreteVAE, anneals the Gumbel temperature (:40-45), forward with reconstruction loss (:48-56),
tf.train.AdamOptimizer(lr) semantics + mean over replicas (CrossShardOptimizer, :58-66), loss/image summaries
(:68-107).  predict raises NotImplementedError as upstream (:30-31)."""
import logging

import torch

from .estimator import CheckpointSaverHook, EstimatorSpec, latest_checkpoint
from .utils import ModeKeys, SummaryWriter, mode_to_str
from .vae_tf import DiscreteVAE
from .vae_tf.kl import kl_log_lines, resolve_kl_options
from .vae_tf.vq import resolve_vq_options, vq_log_lines
from .vae_tf.vq_ema import resolve_vq_ema_options, vq_ema_log_lines


def _dist_info():
    from .dp import dist_setup
    return dist_setup()    # (world, rank, process group, RCCL communicator behind the C ABI or None)


def temperature_schedule(step, params):
    """reference model_fns_tf.py:40-45."""
    if params.get("temp_anneal_steps", None):
        warmup_frac = min(float(step) / params["temp_anneal_steps"], 1.0)
        return params["temp_start"] - warmup_frac * (params["temp_start"] - params["temp"])
    t = params.get("temp")
    return 1.0 if t is None else t


def _stat_scalars(model, loss):
    """loss_recon, loss_kl, kl_weight (beta_t of the forward just run) and the codebook statistics, as floats: what the train
    summaries and eval_metrics carry with "codebook_stats" on or kl_loss_weight > 0 (one DiscreteVAE.codebook_stats() call)"""
    st = model.codebook_stats()
    if model.vq_on:      # vae_tf/vq.py STAT_SCALARS: no posterior, so no kl and no perplexity_soft
        out = dict(loss_recon=float(model.loss_recon[0]), loss_vq=float(model.loss_vq[0]), perplexity_hard=st["perplexity_hard"],
                   codes_used_frac=st["codes_used_frac"])
        if "vq_restarts" in st:      # vae_tf/vq_ema.py EMA_STAT_SCALARS: only with the EMA codebook
            out.update(vq_restarts=float(st["vq_restarts"]), codes_idle=float(st["codes_idle"]))
        return out
    on = model.kl_weight > 0
    return dict(loss_recon=float(model.loss_recon[0]) if on else float(loss), loss_kl=st["kl"],
                kl_weight=float(model.kl_weight_t) if on else 0.0, perplexity_soft=st["perplexity_soft"],
                perplexity_hard=st["perplexity_hard"], codes_used_frac=st["codes_used_frac"])


def _build(params, mode_str):
    kl = resolve_kl_options(params)       # ValueError naming the key, before any device work
    vq = resolve_vq_options(params)
    world, rank, pg, comm = _dist_info()
    ema = resolve_vq_ema_options(params, world=world)
    H = params["dataset"]["image_size"]
    gbs = params[f"{mode_str}_batch_size"]
    assert gbs % world == 0
    n_channels = params.get("input_channels") or 3
    model = DiscreteVAE(
        num_tokens=params["num_tokens"],
        dim=params["n_embd"],              # None in the VAE configs; unused by the tf VAE
        hidden_dim=params["hidden_dim"],
        input_channels=n_channels,
        convblocks=params.get("convblocks") or [(3, 64), (3, 128), (3, 256)],
        recompute_grad=params.get("recompute_grad") or False,
        use_bf16=params.get("use_bf16") or False,
        stack_factor=params.get("stack_factor") or 1,
        dimensions=H, batch_size=gbs // world, mode=mode_str, process_group=pg, world_size=world, comm=comm,
        kl_loss_weight=kl.kl_loss_weight, kl_anneal_steps=kl.kl_anneal_steps, quantizer=vq.quantizer, vq_commitment=vq.vq_commitment,
        vq_ema_decay=ema.vq_ema_decay, vq_restart_after=ema.vq_restart_after or None,
        vq_restart_seed=ema.vq_restart_seed if ema.vq_restart_after else None)
    for line in (vq_log_lines(vq, model.num_tokens, model.grid, model.n_hid) or kl_log_lines(kl, model.num_tokens, model.grid)) + \
            vq_ema_log_lines(ema, model.num_tokens):
        logging.getLogger("dalle_mtf_amd").info("%s %s", mode_str, line)
    ck = latest_checkpoint(params["model_path"]) if params.get("model_path") else None
    if ck is not None:
        model.load_state_dict(torch.load(ck, map_location="cpu"))
    else:
        model.init_params(seed=params.get("seed") or 4321)
    if world > 1:
        import torch.distributed as dist
        for buf in (model.p, model.m, model.v):
            model.reducer.broadcast(buf, root=0)
        box = [model.global_step]
        dist.broadcast_object_list(box, src=0, group=pg)
        model.global_step = int(box[0])
        model.refresh_compute_copies(cast=True)
    saver = CheckpointSaverHook(params.get("model_path"), params.get("steps_per_checkpoint"), model.state_dict,
                                max_to_keep=params.get("max_checkpoints") or 5, is_chief=(rank == 0))
    writer = SummaryWriter(params["model_path"]) if (params.get("model_path") and rank == 0) else None
    return dict(model=model, saver=saver, writer=writer, rank=rank)


def vae_model_fn(features, labels, mode, params):
    mode_str = mode_to_str(mode)
    if mode == ModeKeys.PREDICT:
        raise NotImplementedError
    assert mode in (ModeKeys.TRAIN, ModeKeys.EVAL)
    kl = resolve_kl_options(params)
    stats_on = kl.codebook_stats or kl.kl_loss_weight > 0 or resolve_vq_options(params).quantizer == "vq"
    key = f"_vae_state_{mode_str}"
    if params.get(key) is None:
        if mode == ModeKeys.EVAL and params.get("_vae_state_train") is not None and \
                params["eval_batch_size"] == params["train_batch_size"]:
            params[key] = params["_vae_state_train"]
        else:
            params[key] = _build(params, mode_str)
    st = params[key]
    model = st["model"]
    model.mode = mode_str
    if mode == ModeKeys.EVAL and st is not params.get("_vae_state_train"):
        tr = params.get("_vae_state_train")       # a separately sized eval model scores the CURRENT weights
        if tr is not None:
            if st.get("_synced_step") != tr["model"].global_step:
                model.p.copy_(tr["model"].p)
                model.global_step = tr["model"].global_step
                model.refresh_compute_copies(cast=True)
                st["_synced_step"] = tr["model"].global_step
        else:
            ck = latest_checkpoint(params["model_path"]) if params.get("model_path") else None
            if ck is not None and st.get("_synced_ckpt") != ck:
                model.load_state_dict(torch.load(ck, map_location="cpu"))
                st["_synced_ckpt"] = ck
    train_gumbel = params.get("train_gumbel_hard")
    eval_gumbel = params.get("eval_gumbel_hard")
    train_gumbel = True if train_gumbel is None else train_gumbel
    eval_gumbel = True if eval_gumbel is None else eval_gumbel
    gumbel = train_gumbel if mode == ModeKeys.TRAIN else eval_gumbel
    temp = temperature_schedule(model.global_step, params)
    denormalize = lambda x: (x + 1) / 2          # reference model_fns_tf.py:71,83
    imgs = features["inputs"] if isinstance(features, dict) else features
    if mode == ModeKeys.EVAL:
        loss, reconstruction = model.forward(features, return_recon_loss=True, temperature=temp, hard_gumbel=gumbel, need_grad=False)
        if st["writer"] is not None and float(loss) < 1e-9:      # the reference's record_if(loss < 1e-9) gate (:88)
            st["writer"].images(model.global_step, "eval/input_image", denormalize(imgs))
            st["writer"].images(model.global_step, "eval/reconstruction_image", denormalize(reconstruction))
        metrics = {"_loss": loss}
        if stats_on:
            metrics.update(_stat_scalars(model, loss))
        return EstimatorSpec(mode=mode, loss=loss, eval_metrics=metrics)

    # TRAIN: forward + backward + optimizer run inside train_op as ONE step (DiscreteVAE.train_step: a replayed HIP graph on a
    # single GPU); spec.loss is the device scalar that step fills in -- the loss of this batch before the update, as upstream.
    def train_op():
        model.train_step(features, params["lr"], hard_gumbel=gumbel, temperature=temp)
        return model.global_step

    host_call = None
    if st["writer"] is not None:      # rank 0 only: loss (+ temperature), input and reconstruction images (reference :68-78)
        def host_call_fn(step, loss, temperature, input):
            extra = _stat_scalars(model, loss) if stats_on else {}      # outside the captured step, only where something is logged
            st["writer"].scalars(step, loss=loss, temperature=temperature, **extra)
            st["writer"].images(step, "input_image", denormalize(input))
            st["writer"].images(step, "reconstruction_image", denormalize(model.reconstruction()))   # of the step just run
        host_call = (host_call_fn, {"loss": model.loss[0], "temperature": temp, "input": imgs})
    return EstimatorSpec(mode=mode, loss=model.loss[0], train_op=train_op, host_call=host_call, training_hooks=[st["saver"]])
