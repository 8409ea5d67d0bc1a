"""Entry point: ``python wavernn_score.py --target a.wav --test b.wav`` rates a vocoded wav against its target on the device."""
from tacotronv2_wavernn_chinese_amd.score import main

if __name__ == "__main__":
    main()
