"""What the command-line entry points share: the model and the watermarker as the flags of ``generate.get_parser`` describe them
(the reference's dispatch, generate.py:319-345).  ``generate.py`` generates with them, ``detect.py`` detects."""
from __future__ import annotations


def build_model(args, device, seed):
    """The wrapper of ``--model`` (checkpoints from ``--modelpath``, or seeded random-init weights with ``--synthetic``) with the
    tokenizer patches of ``--encoder_ft_ckpt`` / ``--decoder_ft_ckpt`` applied."""
    from .models.chameleon_wrapper import ChameleonARMMWrapper
    from .models.rar_wrapper import RarARMMWrapper
    from .models.taming_wrapper import TamingARMMWrapper
    from .utils import synth
    from .utils.utils import update_weights

    if args.model == "taming":
        if args.synthetic and args.synthetic_config == "harness":
            gcfg, vcfg = synth.GPTConfig(**synth.HARNESS_GPT), synth.VQConfig(**synth.HARNESS_VQ)
            model = TamingARMMWrapper(None, gpt_cfg=gcfg, vq_cfg=vcfg, gpt_state=synth.synth_gpt_state(gcfg, 21, "cpu", 40.0),
                                      vq_state=synth.synth_vq_state(vcfg, 21, "cpu"), device=device,
                                      max_batch=min(args.batch_size, 128))
        elif args.synthetic:
            model = TamingARMMWrapper.synthetic(synth.TAMING_GPT, synth.TAMING_VQ, seed=0, device=device,
                                                max_batch=min(args.batch_size, 128))
        else:
            model = TamingARMMWrapper(args.modelpath, device=device, max_batch=min(args.batch_size, 128))
    elif args.model == "rar":
        if args.synthetic:
            model = RarARMMWrapper.synthetic(device=device, max_batch=min(args.batch_size, 64))
        else:
            model = RarARMMWrapper(args.modelpath, device=device, max_batch=min(args.batch_size, 64))
    else:
        if args.synthetic:
            model = ChameleonARMMWrapper.synthetic(seed=seed, device=device, max_batch=min(args.batch_size, 16))
        else:
            model = ChameleonARMMWrapper(args.modelpath, seed, device=device, max_batch=min(args.batch_size, 16))
    model.noise_device = args.noise_device
    # Patch model: enc and/or dec (the reference's own calls, generate.py:327-332; all three tokenizers expose the handles)
    if args.encoder_ft_ckpt is not None and args.encoder_ft_ckpt != "none":
        update_weights(model.get_image_tokenizer().encoder, args.encoder_ft_ckpt)
    if args.decoder_ft_ckpt is not None and args.decoder_ft_ckpt != "none":
        update_weights(model.get_image_tokenizer().decoder, args.decoder_ft_ckpt)
    return model


def build_watermarker(args, model):
    """The watermarker of ``--wm_method`` over the model's vocabulary (None for ``none``)."""
    vocab_size = model.get_total_vocab_size()
    if args.wm_method == "gentime":
        from .watermarking.gentime_watermark import GentimeWatermark, SeedStrategy, SplitStrategy
        return GentimeWatermark(model.get_vq(), vocab_size, SeedStrategy(args.wm_seed_strategy),
                                SplitStrategy(args.wm_split_strategy), args.wm_context_size, args.wm_delta,
                                args.wm_gamma, model.device)
    if args.wm_method == "gumbel":
        # RAR ignores gen_params (as in the reference): temperature 1.0, no top-p / top-k (--top_k / --top_p default to Taming's)
        from .watermarking.gumbel_watermark import GumbelWatermark
        return GumbelWatermark(vocab_size, seed=args.wm_gumbel_seed, temperature=1.0, top_p=0.0, top_k=0, device=model.device,
                               ngram=args.wm_context_size)
    if args.wm_method == "custom":
        # a reference-style watermarker from the user's own code: spawn_logit_processor(), detect(codes), __str__ -- the wrappers run
        # its processor through the engines' hooked generation mode
        import importlib
        module, _, name = args.wm_factory.partition(":")
        return getattr(importlib.import_module(module), name)(model, args)
    return None


def build_sync_manager(args, device):
    """The synchronisation layer of ``--sync true`` (generate.py:407-410 of the reference): the networks ``--syncpath`` names, or what
    ``--sync_factory pkg.module:callable`` returns -- a manager (add_sync / remove_sync) as it is, a WAM-like object (embed / detect)
    wrapped into a WamSync so that its geometry fit runs on the device.  None without ``--sync``."""
    if not getattr(args, "sync", False):
        return None
    from .watermarking.synchronization import SyncManager, WamSync
    factory = getattr(args, "sync_factory", None)
    # --sync_embedder native: add_sync's embedder from the checkpoint's embedder.* tensors on the device (wam_embedder.py)
    native = {"embedder": "native"} if getattr(args, "sync_embedder", "torch") == "native" else {}
    # --sync_extractor native: remove_sync's extractor from the checkpoint's detector.* tensors on the device (wam_extractor.py)
    if getattr(args, "sync_extractor", "torch") == "native":
        native["extractor"] = "native"
    if not factory:
        if native:
            return SyncManager(args.syncpath, device, sync=WamSync(args.syncpath, device, **native))
        return SyncManager(args.syncpath, device)
    import importlib
    module, _, name = factory.partition(":")
    made = getattr(importlib.import_module(module), name)(args, device)
    if hasattr(made, "add_sync") and hasattr(made, "remove_sync"):
        return made if isinstance(made, SyncManager) else SyncManager(args.syncpath, device, sync=made)
    if hasattr(made, "embed") and hasattr(made, "detect"):
        return SyncManager(args.syncpath, device, sync=WamSync(args.syncpath, device, wam=made, **native))
    raise TypeError(f"--sync_factory {factory}: {type(made).__name__} has neither add_sync / remove_sync nor embed / detect")
