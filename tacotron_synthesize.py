"""Entry point with the reference's script name: ``python tacotron_synthesize.py --pinyin "ni3 hao3 ." --symbols train.txt --checkpoint taco.npz``."""
from tacotronv2_wavernn_chinese_amd.tacotron import main

if __name__ == "__main__":
    main()
