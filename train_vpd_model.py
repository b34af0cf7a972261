#!/usr/bin/env python3
"""Drop-in for reference train_vpd_model.py (same flags, files and bookkeeping; the
student's arithmetic runs on libvpdhip).  Extra, optional flags: --synthetic N (no
dataset files needed), torchrun for multi-GPU data parallelism, and --state_frequency N /
--resume / --seed S to continue a run from <save_dir>/train_state.pt."""
import argparse
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from vpd_amd import checkpoint as ckpt
from vpd_amd import paths as dataset_paths
from vpd_amd.data import RGB_MEAN_STD, SyntheticCrops, TeacherEmbDataset, load_tennis_default
from vpd_amd.io import store_json
from vpd_amd.models.rgb import RGBF_EmbeddingModel
from vpd_amd.trainer import ModelTrainer

DATASETS = ['tennis', 'fs', 'fx', 'penn', 'diving48']


def get_args():
    parser = argparse.ArgumentParser()
    parser.add_argument('dataset', type=str, choices=DATASETS)
    parser.add_argument('--save_dir', type=str, required=True)
    parser.add_argument('--checkpoint_frequency', type=int)
    parser.add_argument('--num_epochs', type=int, default=1000)
    parser.add_argument('--batch_size', type=int, default=100)
    parser.add_argument('--learning_rate', type=float, default=0.0005)
    parser.add_argument('--img_dim', type=int, default=128)
    parser.add_argument('--flow_img', type=str)
    parser.add_argument('--motion', action='store_true')
    parser.add_argument('--encoder_arch', type=str, default='resnet34')
    parser.add_argument('--model_select_window', type=int, default=5)
    parser.add_argument('--pretrained', action='store_true')
    parser.add_argument('--no_test_video', action='store_true')
    parser.add_argument('--min_pose_score', type=float)
    dataset_group = parser.add_mutually_exclusive_group()
    dataset_group.add_argument('--emb_dir', type=str)
    dataset_group.add_argument('--penn_dir', type=str)
    # extensions (not in the reference)
    parser.add_argument('--synthetic', type=int, help='train on N seeded synthetic crops per epoch')
    parser.add_argument('--synthetic_emb_dim', type=int, default=128)
    parser.add_argument('--gpu_augment', action='store_true',
                        help='(default behaviour, kept for compatibility) loaders hand over decoded u8 crops; ColorJitter / '
                             'mask noise / RandomResizedCrop / normalisation run on the GPU (vpd_amd/augment.py)')
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16'],
                        help='(this build) element type of the HIP path: bf16 (default, no loss scaling) or fp16 -- the reference\'s own '
                             'GPU precision (fp16 autocast + GradScaler), here with a static loss scale (vpd_amd.models.util.LossScaler)')
    parser.add_argument('--loss_scale', default='static', choices=['static', 'dynamic'],
                        help='(this build, --dtype fp16 only) static: a fixed loss scale of 256 (default); dynamic: the reference\'s '
                             'GradScaler() -- steps with inf / NaN gradients are skipped and the scale halved, doubled after 2000 '
                             'clean steps -- decided on the device (vpd_amd.models.util.DynamicLossScaler)')
    parser.add_argument('--ema_decay', type=float,
                        help='(this build) keep an exponential moving average of the weights with this decay: every epoch also '
                             'validates the averaged weights (val_ema in loss.json), best_epoch_ema.* is chosen by the moving '
                             'average of val_ema, and every checkpoint is written a second time as <name>_ema.*')
    parser.add_argument('--ema_warmup', action='store_true',
                        help='(this build, with --ema_decay) decay = min(ema_decay, (1 + t) / (10 + t)) after t updates')
    parser.add_argument('--clip_grad_norm', type=float,
                        help='(this build) torch.nn.utils.clip_grad_norm_ with this max_norm before every optimizer step, decided '
                             'on the device; every epoch prints grad_norm_max and clipped_steps and adds them to loss.json')
    parser.add_argument('--accum_steps', type=int,
                        help='(this build) gradient accumulation: one optimizer step per this many batches (and at the last batch '
                             'of an epoch), i.e. an effective batch of accum_steps x batch_size; the loss is a sum over crops, so '
                             'the gradients are summed, not averaged')
    parser.add_argument('--weight_decay', type=float,
                        help='(this build) AdamW weight decay (default 0.01, torch\'s)')
    parser.add_argument('--no_bn_bias_decay', action='store_true',
                        help='(this build) no weight decay on BatchNorm weights / biases and linear biases: a parameter group of '
                             'their own with weight_decay 0 (ModelTrainer.param_groups)')
    parser.add_argument('--backbone_lr_scale', type=float,
                        help='(this build) the head (fc + motion head) runs at --learning_rate, everything else at this factor '
                             'times it: the --pretrained fine-tuning recipe')
    parser.add_argument('--state_frequency', type=int,
                        help='(this build) write <save_dir>/train_state.pt -- everything --resume needs: weights, optimizer moments '
                             'and step, loss scaler, EMA, clip statistics, random number generators, loss history, split seed -- '
                             'after every N-th epoch and after the last one')
    parser.add_argument('--resume', action='store_true',
                        help='(this build) continue the run in --save_dir from its train_state.pt at the epoch after the stored one; '
                             'every argument but --num_epochs, --checkpoint_frequency and --state_frequency must be the stored run\'s')
    parser.add_argument('--seed', type=int,
                        help='(this build) seed torch (CPU and device), random and numpy, and the train/val split')
    parser.add_argument('--no_augment', action='store_true',
                        help='escape hatch: fp32 batches from the CPU loaders with h-flips only -- NOT the reference '
                             'recipe, whose datasets always augment (vpd_dataset/common.py:85-92)')
    args = parser.parse_args()
    if args.loss_scale == 'dynamic' and args.dtype != 'fp16':
        parser.error('--loss_scale dynamic needs --dtype fp16 (bf16 trains without a loss scale)')
    if args.ema_decay is not None and not 0.0 <= args.ema_decay <= 1.0:
        parser.error('--ema_decay must be in [0, 1]')
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0.0:
        parser.error('--clip_grad_norm must be > 0')
    if args.ema_warmup and args.ema_decay is None:
        parser.error('--ema_warmup needs --ema_decay')
    if args.accum_steps is not None and args.accum_steps < 1:
        parser.error('--accum_steps must be >= 1')
    if args.weight_decay is not None and not args.weight_decay >= 0.0:
        parser.error('--weight_decay must not be negative')
    if args.backbone_lr_scale is not None and not args.backbone_lr_scale >= 0.0:
        parser.error('--backbone_lr_scale must not be negative')
    if args.state_frequency is not None and args.state_frequency < 1:
        parser.error('--state_frequency must be >= 1')
    return args


def get_moving_avg_loss(losses, n, key):
    return np.mean([l[key] for l in losses[-n:]])


def load_dataset(dataset, dataset_kwargs, emb_dir, penn_dir, no_test_video):
    if dataset == 'penn':
        raise NotImplementedError('PennDataset reads a hard-coded private path in the reference (out of scope)')
    if no_test_video:          # hold the downstream test videos out of distillation (train_vpd_model.py:125-156)
        from vpd_amd.splits import get_test_prefixes
        dataset_kwargs['exclude_prefixes'] = get_test_prefixes(dataset)
    if emb_dir is None:
        emb_dir = os.path.join(dataset_paths.ROOT[dataset], 'embs')
    if dataset == 'tennis':          # per-player crop directories, split over clips (train_vpd_model.py:121-128)
        return load_tennis_default(emb_dir, dataset_paths.CROPS[dataset], **dataset_kwargs)
    return TeacherEmbDataset.load_default(emb_dir, dataset_paths.CROPS[dataset], **dataset_kwargs)


def main(dataset, num_epochs, batch_size, learning_rate, img_dim, flow_img, motion, encoder_arch, save_dir,
         model_select_window, checkpoint_frequency, pretrained, emb_dir, penn_dir, no_test_video, min_pose_score,
         synthetic=None, synthetic_emb_dim=128, gpu_augment=False, no_augment=False, dtype='bf16', loss_scale='static', ema_decay=None,
         ema_warmup=False, clip_grad_norm=None, weight_decay=None, no_bn_bias_decay=False, backbone_lr_scale=None,
         accum_steps=None, state_frequency=None, resume=False, seed=None):
    run_args = dict(locals())      # what --resume compares with the stored run's (vpd_amd.checkpoint.check_resume_args)
    stored = None
    if resume:      # everything that can be refused is refused here, before any GPU work
        state_path = ckpt.check_resume_dir(save_dir)
        stored = ckpt.read_state(state_path)
        ckpt.check_resume_args(stored['extra']['args'], run_args)
        if stored['extra']['epoch'] >= num_epochs:
            print('Nothing left to do: {} holds epoch {} of {}'.format(state_path, stored['extra']['epoch'], num_epochs))
            return
    if seed is not None:
        import random
        torch.manual_seed(seed)      # (CPU and every device)
        random.seed(seed)
        np.random.seed(seed % 2 ** 32)
    device = 'cuda'
    # The reference builds train AND val datasets with augment=True (vpd_dataset/single_frame.py:267-272,
    # common.py:85-92): ColorJitter, mask noise, RandomResizedCrop and flips are part of the recipe, so they are the
    # default here too and run on the device; --no_augment is the only way to switch them off.
    gpu_augment = not no_augment
    rank, world = 0, 1
    if 'RANK' in os.environ and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        torch.distributed.init_process_group(os.environ.get('VPD_DIST_BACKEND', 'nccl'))      # 'nccl' = RCCL
    # save_dir must not exist (train_vpd_model.py:221).  Rank 0 creates it FIRST and tells the others, so that every
    # rank leaves together instead of waiting in a collective for a rank that has raised
    made = [None, int.from_bytes(os.urandom(4), 'little') if seed is None else seed]       # [makedirs error or None, split seed]
    if rank == 0 and not resume:
        try:
            os.makedirs(save_dir)
        except OSError as e:
            made[0] = repr(e)
    split_seed = None
    if world > 1:
        # one train/val split for all ranks (the reference's train_test_split is unseeded, vpd_dataset/
        # single_frame.py:263: a split per rank would train the shared weights on other ranks' validation frames)
        torch.distributed.broadcast_object_list(made, src=0)
        split_seed = made[1]
    elif state_frequency is not None or seed is not None:
        split_seed = made[1]      # a run that can be continued must be able to draw the same split again
    if resume:
        split_seed = stored['extra']['split_seed']
    if made[0] is not None:
        if world > 1:
            torch.distributed.destroy_process_group()
        raise FileExistsError('cannot create save_dir {!r}: {}'.format(save_dir, made[0]))
    rgb_mean_std = RGB_MEAN_STD['resnet' if pretrained else dataset]

    if synthetic is not None:
        use_flow = flow_img is not None
        emb_dim = synthetic_emb_dim
        mk = lambda n, seed: SyntheticCrops(n, 5 if use_flow else 3, img_dim, emb_dim, motion, rgb_mean_std, seed,
                                            raw_u8=gpu_augment)
        train_dataset, val_dataset = mk(synthetic, 1 + rank), mk(max(synthetic // 5, 1), 1001 + rank)
    else:
        dataset_kwargs = {'img_dim': img_dim, 'flow_img_name': flow_img, 'embed_time': motion,
                          'rgb_mean_std': rgb_mean_std, 'target_len': 20000 // world, 'split_seed': split_seed}
        if min_pose_score is not None:
            dataset_kwargs['min_pose_score'] = min_pose_score
        train_dataset, val_dataset, emb_dim = load_dataset(dataset, dataset_kwargs, emb_dir, penn_dir, no_test_video)
        train_dataset.raw_u8 = val_dataset.raw_u8 = gpu_augment
        train_dataset.augment = val_dataset.augment = True      # flips stay on with --no_augment (the CPU float path)

    if rank == 0:
        print('Device:', device)
        print('Num epochs:', num_epochs)
        print('Batch size:', batch_size)
        print('Image dim:', img_dim)
        print('Use flow:', flow_img is not None)
        print('Embed time:', motion)
        print('Encoder arch:', encoder_arch)
        print('Dataset:')
        print('', 'Train images:', len(train_dataset))
        print('', 'Val images:', len(val_dataset))
        print('', 'Embedding dim:', emb_dim)
        print('', 'Min pose score:', min_pose_score)

    num_load_workers = min(os.cpu_count(), 8)
    train_loader = DataLoader(train_dataset, batch_size, shuffle=True, num_workers=num_load_workers,
                              persistent_workers=False, pin_memory=True)
    val_loader = DataLoader(val_dataset, batch_size, num_workers=num_load_workers, persistent_workers=False,
                            pin_memory=True)

    encoder = RGBF_EmbeddingModel(encoder_arch, emb_dim, flow_img is not None, device, pretrained=pretrained, dtype=dtype)
    augmenter = None
    if gpu_augment:
        from vpd_amd.augment import CropAugmenter
        augmenter = CropAugmenter(encoder.device, rgb_mean_std, img_dim, flow_img is not None)
    trainer = ModelTrainer(encoder, motion, augmenter=augmenter, augment=True, ema_decay=ema_decay, ema_warmup=ema_warmup,
                           accum_steps=1 if accum_steps is None else accum_steps)
    if world > 1 and not resume:      # same initial weights on every rank (after the trainer: the motion head is initialised there)
        torch.distributed.broadcast(encoder.engine.params, 0)
        torch.distributed.broadcast(encoder.engine.bn_running, 0)
        encoder.engine.mark_weights_changed()
    # parameter groups only when one of their flags is given: without them one group, the optimizer step of always
    grouping = {}
    if weight_decay is not None:
        grouping['weight_decay'] = weight_decay
    if no_bn_bias_decay:
        grouping['no_bn_bias_decay'] = True
    if backbone_lr_scale is not None:
        grouping['backbone_lr_scale'] = backbone_lr_scale
    param_groups = None
    if grouping:
        param_groups = trainer.param_groups(weight_decay=0.01 if weight_decay is None else weight_decay,
                                            decay_bn_bias=not no_bn_bias_decay,
                                            backbone_lr_scale=1.0 if backbone_lr_scale is None else backbone_lr_scale,
                                            lr=learning_rate)
    optimizer, scaler = trainer.get_optimizer(learning_rate, loss_scale='dynamic' if loss_scale == 'dynamic' else None,
                                              max_grad_norm=clip_grad_norm, param_groups=param_groups)
    dynamic = loss_scale == 'dynamic'
    skipped_before = 0
    clip = clip_grad_norm is not None
    clipped_before = 0

    ema = ema_decay is not None
    losses = []
    best_val_loss = float('inf')
    best_val_ema_loss = float('inf')
    first_epoch = 1
    if resume:      # (the order inside load_state: weights, optimizer, scaler, EMA, clip block, random number generators)
        extra = trainer.load_state(state_path, optimizer, scaler, state=stored)
        losses, first_epoch = list(extra['losses']), extra['epoch'] + 1
        best_val_loss, best_val_ema_loss = extra['best_val_loss'], extra['best_val_ema_loss']
        skipped_before, clipped_before = extra['skipped_before'], extra['clipped_before']
        stored = None
        if rank == 0:
            print('Resuming after epoch {}'.format(first_epoch - 1))
    if rank == 0 and not resume:
        config_ema = {} if not ema else {'ema_decay': ema_decay, 'ema_warmup': ema_warmup}      # (keys only with --ema_decay)
        if clip:
            config_ema['clip_grad_norm'] = clip_grad_norm      # (key only with --clip_grad_norm)
        if accum_steps is not None:
            config_ema['accum_steps'] = accum_steps      # (key only with --accum_steps)
        if state_frequency is not None:
            config_ema['state_frequency'] = state_frequency      # (key only with --state_frequency)
        if seed is not None:
            config_ema['seed'] = seed      # (key only with --seed)
        config_ema.update(grouping)      # (weight_decay / no_bn_bias_decay / backbone_lr_scale: keys only with their flags)
        store_json(os.path.join(save_dir, 'config.json'), {
            'num_epochs': num_epochs, 'batch_size': batch_size, 'learning_rate': learning_rate, 'img_dim': img_dim,
            'use_flow': flow_img is not None, 'motion': motion,
            'embed_time': motion,      # apply_vpd_model.py:102 reads this key; the reference never writes it
            'emb_dim': emb_dim, 'encoder_arch': encoder_arch, 'rgb_mean_std': rgb_mean_std,
            'dtype': dtype,            # not in the reference: element type of the HIP path (bf16 | fp16 + a loss scale)
            'loss_scale': loss_scale if dtype == 'fp16' else None,      # fp16: static (256) | dynamic (GradScaler's rule)
            # not in the reference: which input pipeline produced the loss curves
            'augment': 'device: ColorJitter + mask noise + RandomResizedCrop + flip (reference recipe)' if gpu_augment
                       else 'cpu: h-flip only (--no_augment)', **config_ema})

    loss_file = os.path.join(save_dir, 'loss.json')
    for epoch in range(first_epoch, num_epochs + 1):
        train_loss = trainer.epoch(train_loader, optimizer=optimizer, scaler=scaler)
        if world > 1 and os.environ.get('VPD_DDP_AVG_BN', '0') == '1':      # per-rank BatchNorm statistics -> their mean over ranks
            from vpd_amd.ddp import average_running_stats
            average_running_stats(encoder.engine.bn_running)
        val_loss = trainer.epoch(val_loader)
        losses.append({'epoch': epoch, 'train': train_loss, 'val': val_loss,
                       'dataset_train': [(dataset, train_loss)], 'dataset_val': [(dataset, val_loss)]})
        if clip:      # (keys only with --clip_grad_norm; norm_max starts again at 0 for the next epoch)
            stats = optimizer.clip_stats(reset_max=True)
            losses[-1]['grad_norm_max'] = stats['norm_max']
            losses[-1]['clipped_steps'] = stats['clipped_steps'] - clipped_before
            clipped_before = stats['clipped_steps']
        if ema:      # the same validation pass with the averaged weights
            with trainer.ema_weights():
                losses[-1]['val_ema'] = trainer.epoch(val_loader)
            moving_avg_val_ema_loss = get_moving_avg_loss(losses, model_select_window, 'val_ema')
        moving_avg_val_loss = get_moving_avg_loss(losses, model_select_window, 'val')
        if rank == 0:
            print('Epoch {} - train loss: {:0.4f} [avg: {:0.4f}] val loss: {:0.4f} [avg: {:0.4f}]'.format(
                epoch, train_loss, get_moving_avg_loss(losses, model_select_window, 'train'), val_loss,
                moving_avg_val_loss) + ('' if not dynamic else ' loss scale: {:g} skipped steps: {}'.format(
                    scaler.get_scale(), scaler.skipped_steps - skipped_before)) + ('' if not clip else
                ' grad_norm_max: {:g} clipped_steps: {}'.format(losses[-1]['grad_norm_max'], losses[-1]['clipped_steps'])))
            if ema:
                print('  averaged weights - val loss: {:0.4f} [avg: {:0.4f}]'.format(losses[-1]['val_ema'], moving_avg_val_ema_loss))
            store_json(loss_file, losses)
            if moving_avg_val_loss < best_val_loss:
                print('New best epoch!')
                trainer.save_model(save_dir, 'best_epoch')
            if ema and moving_avg_val_ema_loss < best_val_ema_loss:
                print('New best epoch of the averaged weights!')
                trainer.save_model(save_dir, 'best_epoch', ema=True)
            if checkpoint_frequency is not None and epoch % checkpoint_frequency == 0:
                print('Saving checkpoint: {}'.format(epoch))
                trainer.save_model(save_dir, 'epoch{:04d}'.format(epoch))
                if ema:
                    trainer.save_model(save_dir, 'epoch{:04d}'.format(epoch), ema=True)
        if dynamic:
            skipped_before = scaler.skipped_steps
        best_val_loss = min(moving_avg_val_loss, best_val_loss)
        if ema:
            best_val_ema_loss = min(moving_avg_val_ema_loss, best_val_ema_loss)
        if state_frequency is not None and (epoch % state_frequency == 0 or epoch == num_epochs):
            # after the epoch's bookkeeping; every rank calls (the generator states are gathered), rank 0 writes
            trainer.save_state(os.path.join(save_dir, ckpt.STATE_FILE), optimizer, scaler, extra={
                'epoch': epoch, 'losses': losses, 'best_val_loss': float(best_val_loss), 'best_val_ema_loss': float(best_val_ema_loss),
                'skipped_before': int(skipped_before), 'clipped_before': int(clipped_before), 'split_seed': split_seed,
                'args': run_args})
    if rank == 0:
        print('Saving last epoch: {}'.format(epoch))
        trainer.save_model(save_dir, 'epoch{:04d}'.format(epoch))
        if ema:
            trainer.save_model(save_dir, 'epoch{:04d}'.format(epoch), ema=True)
        print('Done!')
    if world > 1:
        # replicas must hold identical weights (same initial broadcast, same summed gradients, same AdamW): verify
        chk = torch.stack([encoder.engine.params.double().sum(), encoder.engine.params.double().square().sum()])
        lo, hi = chk.clone(), chk.clone()
        torch.distributed.all_reduce(lo, op=torch.distributed.ReduceOp.MIN)
        torch.distributed.all_reduce(hi, op=torch.distributed.ReduceOp.MAX)
        # (a one-shot all-reduce may sum in a rank-dependent order: ulp-level drift is tolerated, a missed
        # broadcast or a skipped bucket is not)
        if bool(((hi - lo).abs() > 1e-4 * hi.abs().clamp_min(1e-30)).any()):
            raise RuntimeError('data-parallel replicas diverged: parameter checksums {} .. {}'.format(
                lo.tolist(), hi.tolist()))
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main(**vars(get_args()))
