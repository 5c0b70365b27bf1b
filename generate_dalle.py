"""generate_dalle.py -- images from captions with a trained DALL-E run (the predict path the reference leaves unfinished):
    python generate_dalle.py --model dalle_coco --from-eval 32 --samples-per-caption 4 --top-p 0.9 --out samples/
Captions come from --caption-ids FILE.npy, --captions FILE.txt or --from-eval N; --guidance-scale S adds classifier-free
guidance; see src/generate.py for the outputs."""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))

from src.generate import generate  # noqa: E402


if __name__ == "__main__":
    generate()
