"""The instantiations of the F(4x4,3x3) conv kernel with the DnCNN's last layer fused in are held to the same static rules
as the plain ones (tools/check_w44_isa.py): their template signature must not drop them out of the tool's name match."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_w44_fused_last_layer_is_checked():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_w44_isa.py')], capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert '0 problem(s)' in out.stdout
    checked = [l.split('checked: ', 1)[1] for l in out.stdout.splitlines() if 'checked: ' in l]
    # <LEAKY = false, NG = 2 / 1, STAMP = false, VAR = 0, FL = true>
    for ng in (1, 2):
        assert any(f'k_mid_wino44ILb0ELi{ng}ELb0ELi0ELb1EEEv' in n for n in checked), checked
    assert len(checked) == 6, checked
