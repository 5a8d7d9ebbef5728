"""kNN video retrieval evaluation (mirror of /root/reference/video_retrieval.py).

    python -m selavi_amd.video_retrieval --dataset synthetic --weights_path ckpt.pth --clip_len 16 --batch_size 8 \
        --train_clips_per_video 2
"""
from .retrieval_utils import average_features, init, load_or_get_features, parse_args, retrieval


def main(args, logger=None, dataset=None, dataset_test=None):
    """Features of the train and test clips, averaged per video, test videos retrieved from the train videos.
    Returns retrieval()'s dictionary."""
    model, dataset, dataset_test = init(args, get_video_encoder_only=True, logger=logger, dataset=dataset,
                                        dataset_test=dataset_test)
    train_features, train_vid_indices, train_labels = load_or_get_features(
        args, dataset, model, logger=logger, mode='train', get_audio=args.get_audio)
    val_features, val_vid_indices, val_labels = load_or_get_features(
        args, dataset_test, model, logger=logger, mode='test', get_audio=args.get_audio)
    print("Averaging features")
    train_features, train_vid_indices, train_labels = average_features(
        args, train_features, train_vid_indices, train_labels, get_audio=args.get_audio, aud_features=None, logger=logger)
    val_features, val_vid_indices, val_labels = average_features(
        args, val_features, val_vid_indices, val_labels, get_audio=args.get_audio, aud_features=None, logger=logger)
    return retrieval(train_features, train_labels, train_vid_indices, val_features, val_labels, val_vid_indices,
                     train_aud_features=None, val_aud_features=None, task='v-v')


if __name__ == '__main__':
    args = parse_args()
    args.get_audio = False
    main(args, logger=None)
