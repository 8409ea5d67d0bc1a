"""Entry point with the reference's script name: ``python wavernn_preprocess.py --wav_dir DIR --out_dir DIR [--hp_file FILE]``."""
from tacotronv2_wavernn_chinese_amd.dataset import main

if __name__ == "__main__":
    main()
